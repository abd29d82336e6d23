// libaten_amd.so: host-side renderer object + C-ABI (include/aten_amd.h) over the HIP kernels.
//
// atn::PathTracing mirrors the public surface of the reference's GPU seam --
// idaten::Renderer / idaten::PathTracing (src/libidaten/kernel/renderer.h:17-179,
// src/libidaten/kernel/pathtracing.cpp:23-153): UpdateSceneData, updateCamera, render, reset --
// with the CPU renderer's semantics (frame passed in, CMJ seeded once per sample).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "../../include/aten_amd.h"
#include "device/kernels.hpp"
#include "device/launch.hpp"
#include "device/svgf.hpp"
#include "device/svgf_gather.hpp"
#include "device/restir.hpp"
#include "device/npr.hpp"
#include "device/npr_advance.hpp"
#include "device/ao.hpp"
#include "device/npr_shadow.hpp"
#include "device/npr_hatching.hpp"
#include "device/volume.hpp"
#include "device/lbvh.hpp"
#include "device/skinning.hpp"
#include "device/tlas.hpp"
#include "device/motion.hpp"
#include "device/taa.hpp"
#include "host/scene_upload.hpp"
#include "host/ibl_precompute.hpp"
#include "host/devbuf.hpp"

namespace atn {

// ---- which streams really run side by side ---------------------------------------------------------------------------
// HIP streams are multiplexed onto a few hardware queues (4 by default; under RCCL that number holds whatever
// GPU_MAX_HW_QUEUES says), chosen by the runtime when a stream is created, and two streams that share a queue execute
// strictly one after the other.  Frames in flight live on one stream per bank: measured with rocprofv3 (tools/trace_queues.py)
// under torch.distributed two of the three bank streams shared a queue -- two frames in flight instead of three, 4.20 ->
// 4.46 ms per frame at full size, and on an 8-way shard the 2-in-flight figure (0.83 instead of 0.67 ms).
// The API does not tell which queue a stream got, so it is MEASURED: two spin kernels of kSpinTicks, one per stream; side by
// side they take one spin, on one queue two (a false "clash" under host jitter only costs a needless replacement).
__global__ void k_spin(unsigned long long ticks)
{
    const unsigned long long t0 = wall_clock64();      // constant 100 MHz counter
    while (wall_clock64() - t0 < ticks) { }
}
constexpr unsigned long long kSpinTicks = 30000;        // 300 us: long against launch + synchronise overhead and host jitter
inline bool streams_run_side_by_side(hipStream_t a, hipStream_t b, bool& ok)
{
    const double spin_us = (double)kSpinTicks / 100.0;
    for (int rep = 0; rep < 3; rep++) {                 // the first round also loads the kernel; one round under the limit settles it
        if (hipStreamSynchronize(a) != hipSuccess || hipStreamSynchronize(b) != hipSuccess) { ok = false; return false; }
        const auto t0 = std::chrono::steady_clock::now();
        hipLaunchKernelGGL(k_spin, dim3(1), dim3(1), 0, a, kSpinTicks);
        hipLaunchKernelGGL(k_spin, dim3(1), dim3(1), 0, b, kSpinTicks);
        if (hipStreamSynchronize(a) != hipSuccess || hipStreamSynchronize(b) != hipSuccess) { ok = false; return false; }
        const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
        ok = true;
        if (us < 1.5 * spin_us) return true;            // two spins on one queue cannot take less than 2 x spin_us
    }
    ok = true;
    return false;
}

// An AO ray list (device/ao.hpp's layout): a frame's rays and their answers, the per-slot work words, the per-pixel state, the per-row
// minima and the counters.  The AO renderer keeps one in the context, NPR hatching's AO base one per bank; the value and depth planes
// are the holder's (the two point them at different buffers).
struct AoRayList {
    DevBuf<float4> ray_o, ray_d, ray_n, ray_res;
    DevBuf<uint32_t> work, row_min, counters, state;
    // would ensure() replace a buffer?  (with frames in flight the caller waits for them first)
    bool would_grow(size_t n_rays, size_t n_slots, int32_t w, int32_t h) const
    {
        return n_rays > ray_o.n || n_slots > work.n || (size_t)w * h > state.n || (size_t)h > row_min.n || !counters.p;
    }
    hipError_t ensure(size_t n_rays, size_t n_slots, int32_t w, int32_t h)
    {
        hipError_t e = hipSuccess;
        for (DevBuf<float4>* b : { &ray_o, &ray_d, &ray_n, &ray_res }) if ((e = b->resize(n_rays)) != hipSuccess) return e;
        if ((e = work.resize(n_slots)) != hipSuccess || (e = state.resize((size_t)w * h)) != hipSuccess) return e;
        if ((e = row_min.resize((size_t)h)) != hipSuccess) return e;
        return counters.resize(kAoCounters);
    }
    // the list's part of a frame's AoArgs
    AoArgs args() const
    {
        AoArgs aa{};
        aa.ray_o = ray_o.p; aa.ray_d = ray_d.p; aa.ray_n = ray_n.p; aa.ray_res = ray_res.p;
        aa.work = work.p; aa.row_min = row_min.p; aa.counters = counters.p; aa.state = state.p;
        return aa;
    }
};

// Orders consecutive frames that share state across the banks' streams: a frame records when it is done with the state, the next one
// waits for that record.  The event is created at the first record; the holder decides when to wait and when the flag is void.
struct FrameFence {
    DevEvent ev;
    bool pending = false;
    hipError_t wait(hipStream_t st) const { return pending ? hipStreamWaitEvent(st, ev, 0) : hipSuccess; }
    hipError_t record(hipStream_t st)
    {
        hipError_t e = ev ? hipSuccess : hipEventCreateWithFlags(&ev.h, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventRecord(ev, st);
        if (e == hipSuccess) pending = true;
        return e;
    }
};

// Frames in flight (atn_set_frames_in_flight): everything a frame's kernels write except the film lives in a BANK --
// path state, queues, counters, tile buffer, and the streams / events the frame runs on.  PathTracing derives from Bank: its
// base IS the current bank; render() rotates it with the spare banks, so frame f + 1 is enqueued on another stream while frame
// f's launch tails (a few long rays keep a handful of waves alive at the end of every trace launch) still run.
// Only the film orders consecutive frames: a frame's k_gather waits for the previous frame's.
struct Bank {
    static constexpr int kMaxBatches = 8;
    DevBuf<float4> ray_o, ray_d, thr, contrib, isect, sh_o, sh_d, sh_c, accum, tile_out;
    DevBuf<float4> sh_w;                    // deferred NEE: {incoming direction, sampler dimension} of the vertex behind a slot's shadow ray
    DevBuf<uint32_t> nee_reached;           // deferred NEE: per slot, the shadow ray reached its light (isect then holds two planes of hit records); these
                                            // and isect's second plane exist only in a bank that has run a deferred frame (run_paths)
    DevBuf<float4> pend;                    // path regeneration: a pixel's previous sample while its last shadow ray is in flight
    DevBuf<float4> rg_frames;               // path regeneration: [frames of the burst][slots] pixel values on their way to the film (k_regen_end)
    DevBuf<uint32_t> done, queue0, queue1, shadow_q, counters;
    DevBuf<uint32_t> rg_counters;           // path regeneration: [3][rg_stages + 3] live paths, shadow rays, fetch cursor of every stage (from stage -1)
    DevBuf<uint32_t> rg_regions;            // path regeneration: what a shade launch hands to the compaction: [2][slots + chunk] entries, counts per chunk and group
    int32_t rg_stages = 0;                  // stages the counters hold (of the bank's last regenerated burst: atn_regen_stage_counts)
    DevBuf<float> ns_depth_s, ns_lit, ns_depth, ns_plane;      // the NPR shadow pre-pass's planes of the bank's last mode-1 frame
    uint32_t ns_slots = 0;
    int32_t ns_w = 0, ns_h = 0;
    // NPR hatching (atn_npr_hatching_set, docs/NPR_HATCHING.md): the first step's plane of a two-step direction, and with the AO base
    // the bank's own AO ray list and per-slot / per-pixel words (device/ao.hpp's layout).  ns_lit holds the source plane of either base.
    DevBuf<float> nh_first;
    AoRayList nh_list;
    uint32_t n_slots = 0;
    int32_t counters_depth = 0;
    uint64_t bank_epoch = 0;        // the scene update this bank's stream is behind (wait_scene_epoch)
    int scene_set = 0;              // id of the scene set this bank's last frame read
    DevEvent ev_read[3];            // [scene set id]: the last frame of this bank that read that set has finished with the scene
    DevStream stream, bstream[kMaxBatches];
    DevEvent ev_fork, ev_join[kMaxBatches], ev_gather;      // ev_gather: the bank's "film updated" event
    int batch_streams_checked = 0;  // bstream[0 .. n-1] of this bank are known to be pairwise concurrent
};

// A caller's motion/depth plane (PathTracing::set_motion_depth): SVGF and ReSTIR keep one each.
struct MotionDepth {
    DevBuf<float4> buf;
    bool is_set = false;
    size_t count = 0;       // elements of the last set / upload (buf.n is the capacity)
};

inline void mat_mul(const float* a, const float* b, float* out)        // mat4::operator*=, mat4.h:140-156
{
    float tmp[16];
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {
            float acc = 0.0f;
            for (int k = 0; k < 4; k++) acc += a[4 * i + k] * b[4 * k + j];
            tmp[4 * i + j] = acc;
        }
    std::memcpy(out, tmp, sizeof(tmp));
}

// MatricesForRendering (pt_params.h:150-185): SVGF and ReSTIR keep one each.
struct FrameMatrices {
    float W2V[16] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1 };
    float V2C[16] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1 };
    float prevW2V[16] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1 };
    void reset_identity() { *this = FrameMatrices(); }
    // MatricesForRendering::Reset = Camera::ComputeCameraMatrices: mat4::lookat(origin, center, up) and
    // mat4::perspective(znear, zfar, vfov, aspect) written into the existing matrices (mat4.h:457-513)
    void advance(const atn_camera_param& camera)
    {
        std::memcpy(prevW2V, W2V, 16 * sizeof(float));
        const float* e = camera.origin; const float* at = camera.center; const float* up = camera.up;
        float z[3] = { e[0] - at[0], e[1] - at[1], e[2] - at[2] };
        float il = 1.0f / std::sqrt(z[0] * z[0] + z[1] * z[1] + z[2] * z[2]);        // glm::normalize = v * inversesqrt(dot(v, v))
        z[0] *= il; z[1] *= il; z[2] *= il;
        float x[3] = { up[1] * z[2] - z[1] * up[2], up[2] * z[0] - z[2] * up[0], up[0] * z[1] - z[0] * up[1] };
        il = 1.0f / std::sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
        x[0] *= il; x[1] *= il; x[2] *= il;
        const float y[3] = { z[1] * x[2] - x[1] * z[2], z[2] * x[0] - x[2] * z[0], z[0] * x[1] - x[0] * z[1] };
        float* m = W2V;
        m[0] = x[0]; m[4] = y[0]; m[8] = z[0];
        m[1] = x[1]; m[5] = y[1]; m[9] = z[1];
        m[2] = x[2]; m[6] = y[2]; m[10] = z[2];
        m[3] = -(x[0] * e[0] + x[1] * e[1] + x[2] * e[2]);
        m[7] = -(y[0] * e[0] + y[1] * e[1] + y[2] * e[2]);
        m[11] = -(z[0] * e[0] + z[1] * e[1] + z[2] * e[2]);
        m[15] = 1;
        const float fH = 1 / std::tan((3.14159265358979323846F * (camera.vfov) / 180.0F) * 0.5f);
        const float fW = fH / camera.aspect;
        float* p = V2C;
        p[0] = fW; p[5] = fH;
        p[10] = camera.zfar / (camera.znear - camera.zfar);
        p[11] = camera.znear * camera.zfar / (camera.znear - camera.zfar);
        p[14] = -1.0f; p[15] = 0.0f;
    }
};

class PathTracing : public Bank {
public:
    std::string last_error;
    int device = 0;
    // A frame's paths are cut into n_batches independent batches (contiguous slot ranges = groups of screen tiles),
    // each with its own queues and counters, and every batch runs its gen -> [trace, shade, shadow] x depth sequence on
    // its own stream.  A trace launch has a size-independent part of ~0.2 ms (ramp-up, and a tail in which a few rays
    // that visit 10x the mean number of nodes keep a handful of waves alive); with several batches in flight the other
    // batches' kernels fill the machine meanwhile.  Measured (sponza_lod 1080p): 6.83 -> 6.58 ms
    // on the whole frame, 4.35 -> 3.71 ms on half of it (the 2-GPU shard), no gain below ~200 K paths per batch.
    static constexpr int kMaxShards = 64;       // screen shards of one node (atn_mgpu_*)
    int n_batches = 3;
    bool batches_forced = false;    // ATEN_AMD_BATCHES / atn_set_path_batches given: no size policy on top
    bool fuse_traces = true;    // shadow(b) + closest(b+1) in one launch (k_trace_fused); ATEN_AMD_FUSE=0 disables (experiments)
    bool env_probe_streams = true;  // ATEN_AMD_PROBE_STREAMS=0: take the bank streams as the runtime hands them out
    bool env_lds_nodes = true;  // small node images are walked from an LDS copy (ATEN_AMD_LDS_NODES=0: from global memory)
    int env_anyhit_twin = 1;    // ATEN_AMD_ANYHIT_TWIN: 0 = no any-hit twins, 1 = where the model says they pay (scene_upload.hpp, kTwinPays), 2 = wherever possible
    int env_anyhit_twin_dirs = 8;   // ATEN_AMD_ANYHIT_TWIN_DIRS: 8 = one twin per direction octant (default), 1 = the one direction-free twin
    bool opt_node_layout = true, opt_planar_lights = true;      // ATEN_AMD_NODE_LAYOUT / ATEN_AMD_PLANAR_LIGHTS at creation; atn_set_upload_options
    bool env_atrous4 = true;    // SVGF a-trous levels with four pixels per thread (k_svgf_atrous4); ATEN_AMD_SVGF_ATROUS4=0: one pixel per thread
    int env_shade_waves = 0;    // ATEN_AMD_SHADE_WAVES=4|5 forces the k_shade_wn flavour (default: plan_pass)
    bool env_shadow_plain = true;       // ATEN_AMD_SHADOW_PLAIN=0 (experiments, tests): DevScene::shadow_plain stays off, every shadow job reads its light record
    bool rr_lookahead_twin = true;      // ATEN_AMD_RR_LOOKAHEAD_TWIN=0 (experiments): doomed rays stop at their first hit on the list as given
    int rr_lookahead = 1;       // ATEN_AMD_RR_LOOKAHEAD / atn_set_rr_lookahead: 0 = off, 1 = render()'s serial passes on scenes that qualify
                                // (counted frames keep the reference's accounting: off), 2 = counted frames too (atn_rr_lookahead_stats)
    int nee_deferral = 0;       // ATEN_AMD_NEE_DEFERRAL / atn_set_nee_deferral: 0 = off (the initial mode: docs/NEE_DEFERRAL.md has the measurement), 1 = every
                                // scene that qualifies, 2 = the policy: scenes that qualify and have infinite lights only (scene_upload.hpp, nee_deferral_class)
    int env_flavour = -1;       // ATEN_AMD_TRACE: 1 = the refill walk, 0 = the plain walk for every launch (default: refill_walk)

    // scene (HBM-resident after UpdateSceneData)
    DevBuf<float4> nodes, vtx_pos, vtx_nml, matrices, texels, carpaint, shade_tris;
    DevBuf<atn_triangle_param> tris;
    DevBuf<atn_object_param> objects;
    DevBuf<DevMaterial> materials;
    DevBuf<atn_light_param> lights;
    DevBuf<float4> light_plane;
    DevBuf<DevTexture> textures;
    DevBuf<atn_toon_param> toon;
    DevBuf<atn_light_param> npr_lights;
    DevBuf<float> screen_shadow;
    DevBuf<uint32_t> texels8;
    DevScene scene{};
    bool has_scene = false, has_camera = false;
    std::vector<int32_t> list_root_link;    // typed root link of every BVH list (top layer = list 0, stored last)
    uint32_t n_planar_lights = 0;           // area lights flagged planar + rigid at upload (scene.planar_lights says whether the flags still hold)
    // What a planar light's flag was derived from (scene_upload.hpp: planar_area_light): the instance's and the mesh's object records,
    // the instance's two matrices, the mesh's triangles and the vertices they name.  An update that leaves ALL of it byte for byte
    // as it was leaves the flag true; any other update drops every flag until the next full upload (never re-derived: the host
    // keeps no copy of the vertices).  r06: a deformation tick (new blob vertices, rebuilt list, same lamp) used to drop them --
    // deformable room 1.97 -> 2.04 ms per frame after the first tick (profiles/r06_rebuilt_layout_bound.jsonl).
    struct PlanarCert {
        int32_t light = -1;             // which light the certificate is for
        int32_t inst_obj = -1, mesh_obj = -1, mtx_id = -1;
        atn_object_param inst{}, mesh{};
        atn_mat4 l2w{}, w2l{};
        uint32_t tri_first = 0, tri_count = 0, vtx_lo = 0, vtx_hi = 0;     // [tri_first, tri_first + tri_count), [vtx_lo, vtx_hi]
    };
    std::vector<PlanarCert> planar_certs;
    void collect_planar_certs(const atn_scene_desc* s, const std::vector<atn_light_param>& lights)
    {
        planar_certs.clear();
        for (size_t i = 0; i < lights.size() && i < s->n_lights; i++) {
            if (!lights[i]._pad) continue;
            PlanarCert c;                                          // (planar_area_light accepted this light: every index below is in range)
            c.light = (int32_t)i;
            c.inst_obj = s->lights[i].arealight_objid;
            c.inst = s->objects[c.inst_obj];
            const atn_object_param* o = &s->objects[c.inst_obj];
            if (o->type == ATN_OBJ_INSTANCE) {
                c.mtx_id = o->mtx_id;
                if (c.mtx_id >= 0) { c.l2w = s->matrices[c.mtx_id]; c.w2l = s->matrices[c.mtx_id + 1]; }
                c.mesh_obj = o->object_id;
                c.mesh = s->objects[c.mesh_obj];
                o = &s->objects[c.mesh_obj];
            }
            c.tri_first = (uint32_t)o->triangle_id; c.tri_count = (uint32_t)o->triangle_num;
            c.vtx_lo = 0xFFFFFFFFu; c.vtx_hi = 0;
            for (uint32_t t = c.tri_first; t < c.tri_first + c.tri_count; t++)
                for (int k = 0; k < 3; k++) {
                    const uint32_t v = (uint32_t)s->triangles[t].idx[k];
                    c.vtx_lo = std::min(c.vtx_lo, v); c.vtx_hi = std::max(c.vtx_hi, v);
                }
            planar_certs.push_back(c);
        }
    }
    // the objects (and, when given, the matrices) of an atn_update_tlas leave every planar light's instance as it was uploaded
    bool planar_certs_survive_objects(const atn_object_param* objs, uint32_t n_objs, const atn_mat4* mtxs, uint32_t n_mtxs) const
    {
        for (const PlanarCert& c : planar_certs) {
            if ((uint32_t)c.inst_obj >= n_objs || std::memcmp(&objs[c.inst_obj], &c.inst, sizeof(atn_object_param)) != 0) return false;
            if (c.mesh_obj >= 0 && ((uint32_t)c.mesh_obj >= n_objs || std::memcmp(&objs[c.mesh_obj], &c.mesh, sizeof(atn_object_param)) != 0)) return false;
            if (c.mtx_id >= 0 && n_mtxs
                && ((uint32_t)c.mtx_id + 1 >= n_mtxs || std::memcmp(&mtxs[c.mtx_id], &c.l2w, sizeof(atn_mat4)) != 0
                    || std::memcmp(&mtxs[c.mtx_id + 1], &c.w2l, sizeof(atn_mat4)) != 0)) return false;
        }
        return true;
    }
    // an atn_update_geometry over these vertex / triangle ranges touches none of a planar light's triangles or vertices
    bool planar_certs_survive_geometry(uint32_t vtx_offset, uint32_t n_vtx, uint32_t tri_offset, uint32_t n_tr) const
    {
        for (const PlanarCert& c : planar_certs) {
            if (n_vtx && vtx_offset <= c.vtx_hi && (uint64_t)vtx_offset + n_vtx > c.vtx_lo) return false;
            if (n_tr && tri_offset < c.tri_first + c.tri_count && (uint64_t)tri_offset + n_tr > c.tri_first) return false;
        }
        return true;
    }
    std::vector<int32_t> list_twin_delta;   // HostSceneImage::list_twin_delta: where each list's any-hit twin starts (0 = none)
    std::vector<HostSceneImage::TlasRef> tlas_refs;     // the top layer's TLAS-leaf records and the lists they enter
    uint32_t top_base = 0, n_host_matrices = 0;
    std::vector<atn_mat4> host_matrices;    // the caller's matrices as last uploaded
    std::vector<atn_object_param> host_objects;     // ... and the objects (atn_tlas_rebuild without objects reads their mtx_id)
    std::vector<uint32_t> list_base, list_bytes, list_tri_leaves, list_inner;   // region of every list in the node image
    uint32_t n_scene_tris = 0, n_scene_vtx = 0, n_scene_mtrls = 0;
    // What atn_update_materials / _lights / _texture / _rendering_config edit (docs/SCENE_EDITS.md): the caller's editable data as
    // last handed in, the planar flag of every uploaded light, the textures' storage records and how much of `texels` is in use.
    SceneSource src;
    std::vector<uint8_t> light_planar;
    std::vector<DevTexture> host_textures;
    size_t n_texels_used = 0;

    // LBVH rebuild scratch (atn_lbvh_*), grown on demand
    struct LbvhScratch {
        DevBuf<uint32_t> codes[2], indices[2], counts, totals, arrived, offs;
        DevBuf<uint8_t> flips;          // per inner node, bit g: twin g swaps the children (k_lbvh_twin_flips)
        DevBuf<int32_t> left, right, parent, first, last;
        DevBuf<atn_bvh_node> ref_nodes;
        DevBuf<LbvhBox> pre, suf, sup;
        DevBuf<atn_triangle_param> tris;     // atn_lbvh_build's own inputs
        DevBuf<float4> vtx;
    } lb;
    uint64_t n_bottom_nodes = 0;
    atn_camera_param camera{};

    // optional samplers (atn_set_sampling_options)
    std::vector<atn_vec4> env_host;         // host copy of the environment map (the tables are built on demand)
    int32_t env_w = 0, env_h = 0;
    float env_multiplyer = 1.0F;
    DevBuf<float> ibl_cdf_v, ibl_cdf_u;
    bool ibl_tables_ready = false;
    int32_t opt_ibl_importance = 0, opt_tex_bilinear = 0;

    // sampler
    DevBuf<uint32_t> seeds;
    uint32_t n_seeds = 0;

    // what of the path state is not per bank (the rest: struct Bank)
    DevBuf<float4> film;
    DevBuf<unsigned long long> nee_stats;   // deferred NEE: {shadow rays cast, rays that reached the light} of the deferred frames since the last reset
    DevBuf<unsigned long long> stats;
    DevBuf<uint32_t> cost, cost_film;       // per-slot / per-pixel {node visits, triangle tests} of the last count_stats frame
    int32_t cost_w = 0, cost_h = 0;
    int32_t film_w = 0, film_h = 0;
    int32_t rank = 0, world = 1;

    static constexpr int kMaxInFlight = 4;      // (5 / 6 / 8 banks with 8 hardware queues: no gain, profiles/r04_variants_shade_waves.txt)
    Bank spare[kMaxInFlight - 1];
    int frames_in_flight = 1, n_spare_ready = 0;
    uint64_t frame_seq = 0;
    // the film is one running mean shared by every bank: its last writer (a render()'s k_gather, or reset()'s clear).  One
    // event owned by the context, NOT by a bank -- svgf_render rotates banks without writing the film, so "the previous
    // bank's ev_gather" is not the film's last writer.  (A wait refers to the record that precedes it; re-recording is fine.)
    DevEvent ev_film;
    bool film_pending = false;

    // the whole bank at once: a member added to Bank rotates with it
    void swap_bank(Bank& b) { std::swap(static_cast<Bank&>(*this), b); }

    int set_frames_in_flight(int n)
    {
        if (n < 1 || n > kMaxInFlight) return fail(ATN_ERR_INVALID_ARG, "frames in flight out of range");
        ATN_HIP(hipSetDevice(device));
        int rc = quiesce();
        if (rc) return rc;
        for (; n_spare_ready < n - 1; n_spare_ready++) {
            Bank& b = spare[n_spare_ready];
            ATN_HIP(hipStreamCreateWithFlags(&b.stream.h, hipStreamNonBlocking));
            ATN_HIP(hipEventCreateWithFlags(&b.ev_fork.h, hipEventDisableTiming));
            ATN_HIP(hipEventCreateWithFlags(&b.ev_gather.h, hipEventDisableTiming));
            for (int k = 0; k < kMaxBatches; k++) {
                ATN_HIP(hipStreamCreateWithFlags(&b.bstream[k].h, hipStreamNonBlocking));
                ATN_HIP(hipEventCreateWithFlags(&b.ev_join[k].h, hipEventDisableTiming));
            }
        }
        // the spare scene sets are only kept current while ticks flip through them: an in-place update (one frame in
        // flight) is not logged, so sets kept across N -> 1 -> N would come back stale.  Re-clone at the next flip.
        if (n != frames_in_flight) drop_alt_set();
        frames_in_flight = n;
        if (n > 1 && env_probe_streams) { int rc2 = separate_bank_streams(n); if (rc2) return rc2; }
        return ATN_OK;
    }

    // Every bank's main stream on a hardware queue of its own (see streams_run_side_by_side): a bank stream that shares its
    // queue with an earlier bank's is replaced by a newly created one, up to kStreamTries times (the rejected ones stay
    // alive until the end, so that the runtime's next choice differs).  Best effort: with fewer queues than banks the last
    // candidates are kept as they are.
    static constexpr int kStreamTries = 12;
    int bank_streams_checked = 0;       // banks 0 .. n-1 are known to be pairwise concurrent
    int n_stream_swaps = 0;             // (diagnostics: atn_get_stream_swaps)
    // st[first .. n-1] each made concurrent with every stream before it in the list (replaced in place when they clash)
    int separate_streams(hipStream_t** st, int n, int first)
    {
        std::vector<hipStream_t> rejected;
        for (int i = (first > 1 ? first : 1); i < n; i++) {
            for (int t = 0; t < kStreamTries; t++) {
                bool clash = false;
                for (int j = 0; j < i && !clash; j++) {
                    bool ok = true;
                    const bool par = streams_run_side_by_side(*st[j], *st[i], ok);
                    if (!ok) { for (auto r : rejected) (void)hipStreamDestroy(r); return fail(ATN_ERR_HIP, "stream probe failed"); }
                    clash = !par;
                }
                if (!clash) break;
                if (t == kStreamTries - 1) break;        // out of tries: keep it
                hipStream_t fresh = nullptr;
                if (hipStreamCreateWithFlags(&fresh, hipStreamNonBlocking) != hipSuccess) break;
                rejected.push_back(*st[i]);
                *st[i] = fresh;
                n_stream_swaps++;
            }
        }
        for (auto r : rejected) (void)hipStreamDestroy(r);
        return ATN_OK;
    }
    // The list the new banks are probed against: the main stream, the caller's side stream if it was handed out already (both
    // FIXED: the caller holds their handles), then the spare banks' streams.
    int separate_bank_streams(int n)
    {
        if (n <= bank_streams_checked) return ATN_OK;
        hipStream_t* st[kMaxInFlight + 1];
        int m = 0;
        st[m++] = &stream.h;
        if (side_stream) st[m++] = &side_stream.h;
        const int fixed = m;
        for (int i = 1; i < n; i++) st[m++] = &spare[i - 1].stream.h;
        const int first = fixed + (bank_streams_checked > 1 ? bank_streams_checked - 1 : 0);
        const int rc = separate_streams(st, m, first);
        if (rc) return rc;
        bank_streams_checked = n;
        return ATN_OK;
    }
    // The batch streams a frame forks into when it is rendered in several batches (run_paths).  LAZY: probed the first time
    // a frame of this bank really forks into that many batches -- most contexts (one batch: the refill walk, frames in flight)
    // never fork.  The probe times spin kernels against each other, so it runs on an IDLE device (quiesce: the other banks'
    // frames would read as a clash and cost stream re-creations in the middle of a frame); the count of probed streams is
    // recorded only when the probe succeeded, and a later, larger batch count probes the additional streams.
    int separate_batch_streams(int nb)
    {
        const int n = nb < 3 ? nb : 3;        // the size policy never uses more than two; three when forced
        if (n <= batch_streams_checked || n < 2) return ATN_OK;
        int rc = quiesce();
        if (rc) return rc;
        hipStream_t* st[kMaxBatches];
        for (int i = 0; i < n; i++) st[i] = &bstream[i].h;
        rc = separate_streams(st, n, batch_streams_checked > 1 ? batch_streams_checked : 1);
        if (rc) return rc;
        batch_streams_checked = n;
        return ATN_OK;
    }

    // the caller's side stream (atn_side_stream): concurrent with every bank stream if a queue is left
    DevStream side_stream;
    hipStream_t get_side_stream()
    {
        // handed out once: the caller holds the handle (a torch ExternalStream, a C++ app's own work); banks created later
        // are probed against it (separate_bank_streams), it is never replaced
        if (side_stream) return side_stream;
        if (hipSetDevice(device) != hipSuccess) return nullptr;
        hipStream_t banks[kMaxInFlight];
        banks[0] = stream;
        for (int i = 1; i < frames_in_flight; i++) banks[i] = spare[i - 1].stream;
        auto clashes = [&](hipStream_t c, bool& ok) {
            for (int j = 0; j < frames_in_flight; j++) {
                if (!streams_run_side_by_side(banks[j], c, ok) || !ok) return true;
            }
            return false;
        };
        std::vector<hipStream_t> rejected;
        for (int t = 0; t < kStreamTries; t++) {
            if (!side_stream && hipStreamCreateWithFlags(&side_stream.h, hipStreamNonBlocking) != hipSuccess) { side_stream.h = nullptr; break; }
            bool ok = true;
            const bool clash = env_probe_streams ? clashes(side_stream, ok) : false;
            if (!ok) break;
            if (!clash || t == kStreamTries - 1) break;
            rejected.push_back(side_stream);
            side_stream.h = nullptr;
        }
        // out of tries (fewer queues than banks + 1): any stream will do
        if (!side_stream && !rejected.empty()) { side_stream.h = rejected.back(); rejected.pop_back(); }
        for (auto r : rejected) (void)hipStreamDestroy(r);
        return side_stream;
    }

    // every frame in flight finished (all banks' streams idle): required before anything but the next render()
    int quiesce()
    {
        ATN_HIP(hipStreamSynchronize(stream));
        for (int i = 0; i < n_spare_ready; i++) ATN_HIP(hipStreamSynchronize(spare[i].stream));
        if (sv_stream) ATN_HIP(hipStreamSynchronize(sv_stream));
        if (scene_stream) ATN_HIP(hipStreamSynchronize(scene_stream));
        film_pending = false;
        ta_fence.pending = false;       // (the display tail runs on one of the streams above)
        sv_prepare_recorded[0] = sv_prepare_recorded[1] = false;
        return ATN_OK;
    }

    // Scene updates between frames (atn_update_geometry / atn_lbvh_rebuild_list / atn_update_tlas) do not stop the host:
    // they are enqueued on the current bank's stream behind the frames in flight (every bank's "film updated" event is
    // its last read of the scene), their host inputs travel through a pinned staging arena, and the next render on every
    // bank waits for `ev_scene`.  The host only ever waits for the staging arena of the PREVIOUS update to drain.
    // With frames in flight the MUTABLE part of the scene (node image, vertices, triangles, shading records, objects,
    // matrices) exists twice: an update is written into the set no recent frame reads, after copying over what the
    // previous update changed in the other one (its dirty ranges, device to device), and only frames enqueued afterwards
    // read it -- so the frames in flight keep running while the next tick's geometry, LBVH and top layer are built.
    // The members below ARE the set being written / read by new frames; `alt` is the other one (allocated at the first
    // update of a scene).  In place, behind all frames, when there is one frame in flight or the caller writes the arrays
    // itself (atn_scene_device_arrays).
    enum SceneBufId { SB_NODES, SB_VTX_POS, SB_VTX_NML, SB_SHADE, SB_MATRICES, SB_TRIS, SB_OBJECTS, SB_COUNT };
    struct SceneRange { int buf; size_t off, bytes; };
    struct SceneSet {
        DevBuf<float4> nodes, vtx_pos, vtx_nml, shade_tris, matrices;
        DevBuf<atn_triangle_param> tris;
        DevBuf<atn_object_param> objects;
        int id = 0;                 // which set this is (banks remember the id their last frame read)
        uint64_t tick = 0;          // the update after which this set was complete
        void release() { nodes.release(); vtx_pos.release(); vtx_nml.release(); shade_tris.release(); matrices.release(); tris.release(); objects.release(); }
    };
    // One set per frame in flight, up to three: the set written by a tick is the one that was current longest ago, so
    // its last readers are (frames in flight) ticks old and have normally finished -- the tick does not wait.
    static constexpr int kMaxSceneSets = 3;
    SceneSet alt[kMaxSceneSets - 1];
    int n_alt = 0;                                  // allocated sets besides the current one
    bool frame_since_update = true, scene_in_place = false;
    int cur_set = 0;                                // id (Bank::scene_set: the set a bank's last frame read)
    uint64_t cur_tick = 0, tick_counter = 0;
    std::vector<SceneRange> log_now;                // what the updates since the last flip wrote into the current set
    struct TickLog { uint64_t tick; std::vector<SceneRange> ranges; };
    std::vector<TickLog> log_hist;                  // the last kMaxSceneSets - 1 finished ticks

    char* set_ptr(int b)
    {
        switch (b) {
        case SB_NODES: return (char*)nodes.p; case SB_VTX_POS: return (char*)vtx_pos.p; case SB_VTX_NML: return (char*)vtx_nml.p;
        case SB_SHADE: return (char*)shade_tris.p; case SB_MATRICES: return (char*)matrices.p; case SB_TRIS: return (char*)tris.p;
        default: return (char*)objects.p;
        }
    }
    static char* alt_ptr(SceneSet& a, int b)
    {
        switch (b) {
        case SB_NODES: return (char*)a.nodes.p; case SB_VTX_POS: return (char*)a.vtx_pos.p; case SB_VTX_NML: return (char*)a.vtx_nml.p;
        case SB_SHADE: return (char*)a.shade_tris.p; case SB_MATRICES: return (char*)a.matrices.p; case SB_TRIS: return (char*)a.tris.p;
        default: return (char*)a.objects.p;
        }
    }
    size_t set_bytes(int b)
    {
        switch (b) {
        case SB_NODES: return nodes.n * sizeof(float4); case SB_VTX_POS: return vtx_pos.n * sizeof(float4); case SB_VTX_NML: return vtx_nml.n * sizeof(float4);
        case SB_SHADE: return shade_tris.n * sizeof(float4); case SB_MATRICES: return matrices.n * sizeof(float4);
        case SB_TRIS: return tris.n * sizeof(atn_triangle_param); default: return objects.n * sizeof(atn_object_param);
        }
    }
    void log_range(int b, size_t off, size_t bytes)
    {
        if (!bytes) return;
        log_now.push_back(SceneRange{ b, off, bytes });
        if (gm_on && (b == SB_VTX_POS || b == SB_MATRICES)) gm_note_range(SceneRange{ b, off, bytes });
    }

    // Geometry motion vectors (atn_set_geometry_motion, device/motion.hpp, docs/MOTION.md).  The GEOMETRY HISTORY: the scene's vertex
    // positions and matrices as the last frame rendered with compute_motion = 2 saw them.  One per context -- SVGF and ReSTIR frames
    // share it, and it belongs to no scene set: every update logs the ranges of SB_VTX_POS / SB_MATRICES it writes (the offsets are
    // the same in every set), and a mode-2 frame copies exactly those, from the set it reads, behind its motion pass.  Frames are
    // ordered through gm_fence: a frame's motion pass reads the history only after the previous frame's copies, and writes it only
    // after the previous frame's reads -- on the device, frame after frame, like the film.
    bool gm_on = false;
    DevBuf<float4> gm_vtx, gm_mtx;
    uint32_t gm_mtx_quads = 0;                  // matrices rows the history holds (scene.mtx_quads when it was last made equal)
    std::vector<SceneRange> gm_dirty;           // written since the last mode-2 frame
    FrameFence gm_fence;            // the last mode-2 frame is done with the history
    DevBuf<float4> gm_ids[2], gm_rs_ids;        // ids planes: SVGF's per hand-over slot, ReSTIR's
    float4* gm_capture = nullptr;               // run_paths: where the frame's bounce-0 hit records go (null: not captured)
    bool gm_sv_ids[2] = { false, false }, gm_rs_has_ids = false;       // the plane holds a frame's ids
    uint64_t gm_stats[3] = {};                  // motion passes, range copies launched, float4s copied (atn_geometry_motion_stats)
    float gm_w2c[16] = {}, gm_prev_w2c[16] = {};    // the camera matrices of the last motion pass (atn_geometry_motion_matrices)

    // A range an update wrote, for the next mode-2 frame.  The list stays short whatever the caller renders in between: a range that
    // an entry already covers is dropped (a tick writes the ranges the tick before it wrote), and a list that still reaches
    // kGmMaxDirty entries is merged -- overlapping ranges joined, then, if need be, one covering range per buffer.
    static constexpr size_t kGmMaxDirty = 64;
    void gm_note_range(const SceneRange& r)
    {
        for (const SceneRange& e : gm_dirty)
            if (e.buf == r.buf && e.off <= r.off && r.off + r.bytes <= e.off + e.bytes) return;
        gm_dirty.push_back(r);
        if (gm_dirty.size() < kGmMaxDirty) return;
        gm_merge_dirty();
        if (gm_dirty.size() < kGmMaxDirty / 2) return;
        std::vector<SceneRange> cover;
        for (const SceneRange& e : gm_dirty) {          // (sorted by buffer and offset)
            if (cover.empty() || cover.back().buf != e.buf) cover.push_back(e);
            else cover.back().bytes = e.off + e.bytes - cover.back().off;
        }
        gm_dirty.swap(cover);
    }
    // sorted by buffer and offset, overlapping and adjoining ranges joined
    void gm_merge_dirty()
    {
        std::sort(gm_dirty.begin(), gm_dirty.end(), [](const SceneRange& a, const SceneRange& b) { return a.buf != b.buf ? a.buf < b.buf : a.off < b.off; });
        size_t k = 0;
        for (size_t i = 0; i < gm_dirty.size(); i++) {
            if (k && gm_dirty[k - 1].buf == gm_dirty[i].buf && gm_dirty[i].off <= gm_dirty[k - 1].off + gm_dirty[k - 1].bytes) {
                const size_t end = std::max(gm_dirty[k - 1].off + gm_dirty[k - 1].bytes, gm_dirty[i].off + gm_dirty[i].bytes);
                gm_dirty[k - 1].bytes = end - gm_dirty[k - 1].off;
            }
            else gm_dirty[k++] = gm_dirty[i];
        }
        gm_dirty.resize(k);
    }

    // the history := the current scene, behind everything in flight (upload, switching on: not per frame)
    int gm_reset_history()
    {
        ATN_HIP(gm_vtx.resize(vtx_pos.n ? vtx_pos.n : 1));
        ATN_HIP(gm_mtx.resize(matrices.n ? matrices.n : 1));
        if (vtx_pos.n) ATN_HIP(hipMemcpyAsync(gm_vtx.p, vtx_pos.p, vtx_pos.n * sizeof(float4), hipMemcpyDeviceToDevice, stream));
        if (matrices.n) ATN_HIP(hipMemcpyAsync(gm_mtx.p, matrices.p, matrices.n * sizeof(float4), hipMemcpyDeviceToDevice, stream));
        ATN_HIP(hipStreamSynchronize(stream));
        gm_mtx_quads = scene.mtx_quads;
        gm_dirty.clear();
        gm_fence.pending = false;
        return ATN_OK;
    }
    int set_geometry_motion(int32_t on)
    {
        ATN_HIP(hipSetDevice(device));
        { int q = quiesce(); if (q) return q; }
        if (!on) {
            gm_on = false; gm_dirty.clear(); gm_fence.pending = false;
            gm_vtx.release(); gm_mtx.release(); gm_ids[0].release(); gm_ids[1].release(); gm_rs_ids.release();
            gm_sv_ids[0] = gm_sv_ids[1] = gm_rs_has_ids = false;
            return ATN_OK;
        }
        if (scene_in_place) return fail(ATN_ERR_UNSUPPORTED, "geometry motion needs to see every scene update: not once the caller writes the scene arrays itself (atn_scene_device_arrays)");
        if (gm_on) return ATN_OK;
        gm_on = true;
        return has_scene ? gm_reset_history() : ATN_OK;
    }
    // A mode-2 frame's motion pass and the history's update, on the frame's stream.  `ma` comes with ids, pos, motion and the camera
    // matrices filled in; the scene and the history are added here.
    int gm_motion_pass(MotionArgs ma, int32_t width, int32_t height)
    {
        if (frames_in_flight > 1) ATN_HIP(gm_fence.wait(stream));
        // another number of matrices (instances added / removed): no previous matrix to pair with -- object motion is zero this frame
        if (scene.mtx_quads != gm_mtx_quads) {
            if (matrices.n > gm_mtx.n) {
                { int q = quiesce(); if (q) return q; }
                ATN_HIP(gm_mtx.resize(matrices.n));
            }
            motion_launch_copy(stream, gm_mtx.p, matrices.p, scene.mtx_quads);
            gm_stats[1]++; gm_stats[2] += scene.mtx_quads;
            gm_mtx_quads = scene.mtx_quads;
            size_t k = 0;
            for (const SceneRange& r : gm_dirty) if (r.buf != SB_MATRICES) gm_dirty[k++] = r;
            gm_dirty.resize(k);
        }
        ma.objects = objects.p; ma.tris = tris.p; ma.h_vtx = gm_vtx.p; ma.h_mtx = gm_mtx.p;
        ma.width = width; ma.height = height;
        ma.n_objects = (uint32_t)objects.n; ma.n_tris = (uint32_t)(n_scene_tris < tris.n ? n_scene_tris : tris.n);
        ma.n_vtx = (uint32_t)(n_scene_vtx < gm_vtx.n ? n_scene_vtx : gm_vtx.n); ma.h_mtx_quads = (uint32_t)(gm_mtx_quads < gm_mtx.n ? gm_mtx_quads : gm_mtx.n);
        motion_launch_geometry(tile_launch(width, height), stream, ma);
        std::memcpy(gm_w2c, ma.w2c, sizeof(gm_w2c)); std::memcpy(gm_prev_w2c, ma.prev_w2c, sizeof(gm_prev_w2c));
        gm_stats[0]++;
        // the history := the scene this frame saw: the union of the logged ranges (two ticks between two frames wrote the same ones)
        gm_merge_dirty();
        for (const SceneRange& r : gm_dirty) {
            DevBuf<float4>& h = r.buf == SB_VTX_POS ? gm_vtx : gm_mtx;
            size_t end = r.off + r.bytes;
            if (end > h.n * sizeof(float4)) end = h.n * sizeof(float4);
            if (end > set_bytes(r.buf)) end = set_bytes(r.buf);
            if (r.off >= end) continue;
            const uint32_t q0 = (uint32_t)(r.off / sizeof(float4)), nq = (uint32_t)((end - r.off) / sizeof(float4));
            motion_launch_copy(stream, h.p + q0, reinterpret_cast<const float4*>(set_ptr(r.buf)) + q0, nq);
            gm_stats[1]++; gm_stats[2] += nq;
        }
        gm_dirty.clear();
        ATN_HIP(hipGetLastError());
        if (frames_in_flight > 1) ATN_HIP(gm_fence.record(stream));
        return ATN_OK;
    }
    void drop_alt_set()
    {
        for (int k = 0; k < n_alt; k++) alt[k].release();
        n_alt = 0; log_now.clear(); log_hist.clear();
    }
    void point_scene_at_current_set()
    {
        scene.nodes = nodes.p; scene.tris = tris.p; scene.shade_tris = shade_tris.p; scene.vtx_pos = vtx_pos.p; scene.vtx_nml = vtx_nml.p;
        scene.objects = objects.p; scene.matrices = matrices.p;
    }
    // switch to the set that was current longest ago (see above); everything is enqueued on `upd`
    int flip_scene_set()
    {
        // the tick that just ended (the updates since the last flip) becomes history
        if (!log_now.empty()) {
            log_hist.push_back(TickLog{ cur_tick, std::move(log_now) });
            log_now.clear();
            if (log_hist.size() > (size_t)(kMaxSceneSets - 1)) log_hist.erase(log_hist.begin());
        }
        const int want = (frames_in_flight < kMaxSceneSets ? frames_in_flight : kMaxSceneSets) - 1;     // sets besides the current one
        SceneSet* t = nullptr;
        if (n_alt < want) {
            // a new set: a clone of the current one
            t = &alt[n_alt];
            ATN_HIP(t->nodes.resize(nodes.n)); ATN_HIP(t->vtx_pos.resize(vtx_pos.n)); ATN_HIP(t->vtx_nml.resize(vtx_nml.n));
            ATN_HIP(t->shade_tris.resize(shade_tris.n)); ATN_HIP(t->matrices.resize(matrices.n));
            ATN_HIP(t->tris.resize(tris.n)); ATN_HIP(t->objects.resize(objects.n));
            for (int b = 0; b < SB_COUNT; b++)
                if (set_bytes(b)) ATN_HIP(hipMemcpyAsync(alt_ptr(*t, b), set_ptr(b), set_bytes(b), hipMemcpyDeviceToDevice, upd));
            // ids 0 .. kMaxSceneSets-1, none in use twice
            bool used[kMaxSceneSets] = {};
            used[cur_set] = true;
            for (int k = 0; k < n_alt; k++) used[alt[k].id] = true;
            for (int id = 0; id < kMaxSceneSets; id++) if (!used[id]) { t->id = id; break; }
            t->tick = cur_tick;
            n_alt++;
        }
        else {
            if (n_alt == 0) return ATN_OK;      // (one frame in flight never gets here)
            t = &alt[0];
            for (int k = 1; k < n_alt; k++) if (alt[k].tick < t->tick) t = &alt[k];
            // the frames that still read it: its writers go behind them
            // (per bank and set, not "the bank's last frame": an older frame of a bank may still be running behind a newer
            // one that reads another set)
            for (int i = 0; i < n_spare_ready; i++)
                if (spare[i].ev_read[t->id]) ATN_HIP(hipStreamWaitEvent(upd, spare[i].ev_read[t->id], 0));
            if (ev_read[t->id]) ATN_HIP(hipStreamWaitEvent(upd, ev_read[t->id], 0));
            // what the ticks since its own wrote into the other sets is missing there: the current set has all of it
#ifndef ATN_DEBUG_NO_REPLAY      /* (the tests' negative control: without the replay test_ticks_touching_different_ranges_are_replayed fails) */
            for (const TickLog& L : log_hist)
                if (L.tick > t->tick)
                    for (const SceneRange& r : L.ranges)
                        ATN_HIP(hipMemcpyAsync(alt_ptr(*t, r.buf) + r.off, set_ptr(r.buf) + r.off, r.bytes, hipMemcpyDeviceToDevice, upd));
#endif
        }
        // swap: the target becomes the members, the old current takes its slot
        nodes.swap(t->nodes); vtx_pos.swap(t->vtx_pos); vtx_nml.swap(t->vtx_nml); shade_tris.swap(t->shade_tris);
        matrices.swap(t->matrices); tris.swap(t->tris); objects.swap(t->objects);
        std::swap(cur_set, t->id);
        t->tick = cur_tick;                 // the old current set is complete up to the tick that just ended
        cur_tick = ++tick_counter;          // the tick being written now
        point_scene_at_current_set();
        return ATN_OK;
    }

    DevEvent ev_scene, ev_stage;
    DevStream scene_stream;            // updates run here when frames are in flight: not behind the newest frame
    hipStream_t upd = nullptr;                      // the stream of the update in progress (scene_stream, or `stream` with one frame in flight)
    uint64_t scene_epoch = 0;                       // (Bank::bank_epoch: the update a bank's stream is behind)
    bool stage_busy = false;
    char* stage_p = nullptr;
    size_t stage_cap = 0, stage_used = 0;

    int begin_scene_update(size_t stage_bytes)
    {
        if (!ev_scene) { ATN_HIP(hipEventCreateWithFlags(&ev_scene.h, hipEventDisableTiming)); ATN_HIP(hipEventCreateWithFlags(&ev_stage.h, hipEventDisableTiming)); }
        if (stage_busy) { ATN_HIP(hipEventSynchronize(ev_stage)); stage_busy = false; }       // the previous update's copies
        stage_used = 0;
        if (stage_bytes > stage_cap) {
            if (stage_p) ATN_HIP(hipHostFree(stage_p));
            stage_p = nullptr; stage_cap = 0;
            const size_t cap = stage_bytes + stage_bytes / 2 + 4096;
            ATN_HIP(hipHostMalloc((void**)&stage_p, cap, hipHostMallocDefault));
            stage_cap = cap;
        }
        if (frames_in_flight > 1 && !scene_stream) ATN_HIP(hipStreamCreateWithFlags(&scene_stream.h, hipStreamNonBlocking));
        upd = frames_in_flight > 1 ? scene_stream : stream;
        if (frames_in_flight > 1 && n_spare_ready > 0 && !scene_in_place) {
            // a frame may be reading the current set: write the other one.  (Several updates in a row -- geometry, LBVH,
            // top layer -- flip once: no frame has been enqueued in between.)
            if (frame_since_update) { int r = flip_scene_set(); if (r) return r; frame_since_update = false; }
            return ATN_OK;
        }
        if (n_alt > 0 && frames_in_flight <= 1) drop_alt_set();   // written in place and unlogged: spare sets would miss this update (set_frames_in_flight quiesced)
        log_now.clear();        // (no other set to replay into)
        // in place, behind every frame in flight: a bank's ev_gather is recorded after its last kernel that reads the scene
        // (the filter stream of pipelined SVGF frames never reads the scene)
        if (upd != stream) {
            for (int i = 0; i < n_spare_ready; i++) if (spare[i].ev_gather) ATN_HIP(hipStreamWaitEvent(upd, spare[i].ev_gather, 0));
            if (ev_gather) ATN_HIP(hipStreamWaitEvent(upd, ev_gather, 0));
        }
        return ATN_OK;
    }
    // host bytes -> device, through the arena (the caller's memory is free again when this returns)
    int stage_copy(void* dst_dev, const void* src_host, size_t bytes)
    {
        if (!bytes) return ATN_OK;
        const size_t off = (stage_used + 63) & ~(size_t)63;
        if (off + bytes > stage_cap) return fail(ATN_ERR_INVALID_ARG, "staging arena too small (internal)");
        std::memcpy(stage_p + off, src_host, bytes);
        stage_used = off + bytes;
        ATN_HIP(hipMemcpyAsync(dst_dev, stage_p + off, bytes, hipMemcpyHostToDevice, upd));
        return ATN_OK;
    }
    int end_scene_update()
    {
        if (stage_used) { ATN_HIP(hipEventRecord(ev_stage, upd)); stage_busy = true; }
        ATN_HIP(hipEventRecord(ev_scene, upd));
        scene_epoch++;
        if (upd == stream) bank_epoch = scene_epoch;       // this bank's stream is already behind the update
        return ATN_OK;
    }
    // with frames in flight: this bank's frame has read the scene for the last time (its ev_gather, and the scene set's ev_read)
    int record_scene_read()
    {
        ATN_HIP(hipEventRecord(ev_gather, stream));
        DevEvent& e = ev_read[scene_set];
        if (!e) ATN_HIP(hipEventCreateWithFlags(&e.h, hipEventDisableTiming));
        ATN_HIP(hipEventRecord(e, stream));
        return ATN_OK;
    }
    // first thing a frame does on its bank's stream
    int wait_scene_epoch()
    {
        if (bank_epoch != scene_epoch && ev_scene) ATN_HIP(hipStreamWaitEvent(stream, ev_scene, 0));
        bank_epoch = scene_epoch;
        scene_set = cur_set;
        frame_since_update = true;
        return ATN_OK;
    }

    // profiling
    float k_ms[ATN_K_MGPU_COUNT] = {};       // (atn_get_kernel_times reports the first ATN_K_COUNT)
    uint32_t k_launches[ATN_K_MGPU_COUNT] = {};
    std::vector<DevEvent> ev_pool;
    struct Span { int kind; size_t e0, e1; };
    static constexpr size_t kMaxSpans = 8192;
    std::vector<Span> spans;
    size_t ev_used = 0;
    hipStream_t prof_stream = nullptr;
    uint64_t host_stats[16] = {};

    int fail(int code, const std::string& msg) { last_error = msg; return code; }

    // ---- analytic spheres (atn_set_sphere_intersection, docs/SPHERES.md) ----
    int sphere_mode = 0;                // context state like the upload options: read by the next atn_upload_scene / atn_update_tlas
    uint32_t n_sphere_leaves = 0;       // top-layer leaves of the uploaded scene the sphere-aware kernels (spheres.hip) test; 0 in mode 0
    // what a scene with sphere leaves cannot be used for (each is a later change): false = go on
    int sph_refuse(const char* what)
    {
        if (!n_sphere_leaves) return ATN_OK;
        return fail(ATN_ERR_UNSUPPORTED, std::string("sphere intersection: ") + what + " (atn_set_sphere_intersection(0) and upload the scene again)");
    }

    int init(int device_ordinal)
    {
        int n = 0;
        hipError_t e = hipGetDeviceCount(&n);
        if (e != hipSuccess || n <= 0) return fail(ATN_ERR_NO_DEVICE, "no HIP device available (libaten_amd has no CPU fallback)");
        if (device_ordinal < 0 || device_ordinal >= n) return fail(ATN_ERR_INVALID_ARG, "device ordinal out of range");
        device = device_ordinal;
        ATN_HIP(hipSetDevice(device));
        ATN_HIP(hipStreamCreateWithFlags(&stream.h, hipStreamNonBlocking));
        for (int k = 0; k < kMaxBatches; k++) {
            ATN_HIP(hipStreamCreateWithFlags(&bstream[k].h, hipStreamNonBlocking));
            ATN_HIP(hipEventCreateWithFlags(&ev_join[k].h, hipEventDisableTiming));
        }
        ATN_HIP(hipEventCreateWithFlags(&ev_fork.h, hipEventDisableTiming));
        ATN_HIP(hipEventCreateWithFlags(&ev_gather.h, hipEventDisableTiming));
        // environment switches (README.md "Environment variables": which are supported controls, which are experiment hooks);
        // read once here, never inside a frame
        if (const char* e = std::getenv("ATEN_AMD_FUSE")) fuse_traces = e[0] != '0';
        if (const char* e = std::getenv("ATEN_AMD_SHADOW_PLAIN")) env_shadow_plain = e[0] != '0';
        if (const char* e = std::getenv("ATEN_AMD_SVGF_ATROUS4")) env_atrous4 = e[0] != '0';     // 0: the one-pixel-per-thread a-trous kernel
        if (const char* e = std::getenv("ATEN_AMD_SHADE_WAVES")) { const int v = std::atoi(e); if (v == 4 || v == 5) env_shade_waves = v; }   // else: plan_pass
        if (const char* e = std::getenv("ATEN_AMD_LDS_NODES")) env_lds_nodes = std::atoi(e) != 0;
        if (const char* e = std::getenv("ATEN_AMD_RR_LOOKAHEAD")) rr_lookahead = std::max(0, std::min(2, std::atoi(e)));
        if (const char* e = std::getenv("ATEN_AMD_NEE_DEFERRAL")) nee_deferral = std::max(0, std::min(2, std::atoi(e)));
        if (const char* e = std::getenv("ATEN_AMD_RR_LOOKAHEAD_TWIN")) rr_lookahead_twin = std::atoi(e) != 0;
        if (const char* e = std::getenv("ATEN_AMD_ANYHIT_TWIN")) env_anyhit_twin = std::max(0, std::min(2, std::atoi(e)));
        if (const char* e = std::getenv("ATEN_AMD_ANYHIT_TWIN_DIRS")) env_anyhit_twin_dirs = std::atoi(e) == 1 ? 1 : 8;
        if (const char* e = std::getenv("ATEN_AMD_NODE_LAYOUT")) opt_node_layout = std::atoi(e) != 0;     // 0: bottom-level records in walk order
        if (const char* e = std::getenv("ATEN_AMD_PLANAR_LIGHTS")) opt_planar_lights = std::atoi(e) != 0; // 0: shadow rays towards area lights always walk to their closest hit
        if (const char* e = std::getenv("ATEN_AMD_PROBE_STREAMS")) env_probe_streams = std::atoi(e) != 0;
        if (const char* e = std::getenv("ATEN_AMD_TRACE")) { env_flavour = e[0] == 'r' ? 1 : 0; }   // 'r'efill / 's'imple
        if (const char* e = std::getenv("ATEN_AMD_BATCHES")) {
            n_batches = std::atoi(e);
            batches_forced = true;
            if (n_batches < 1) n_batches = 1;
            if (n_batches > kMaxBatches) n_batches = kMaxBatches;
        }
        // (the streams a frame's batches run on are probed lazily: separate_batch_streams, run_paths)
        return ATN_OK;
    }

    // Streams, events and buffers go with their wrappers: this class's members in reverse order of declaration (the renderers' state,
    // the update streams, the spare banks), then the base -- the current bank, its main stream among the last.  hipStreamDestroy and
    // hipEventDestroy let queued work finish, and every hipFree waits for the device.
    ~PathTracing() { if (stage_p) (void)hipHostFree(stage_p); }

    // ≙ idaten::Renderer::UpdateSceneData, src/libidaten/kernel/renderer.cpp:12-131
    int UpdateSceneData(const atn_scene_desc* s)
    {
        ATN_HIP(hipSetDevice(device));
        { int q = quiesce(); if (q) return q; }
        drop_alt_set(); cur_set = 0; scene_in_place = false; frame_since_update = true;
        skins.clear();          // a skin is bound to ranges of the scene it was created on
        HostSceneImage img;
        std::string err;
        // (the upload options are context state: the environment was read ONCE, when the context was created; atn_set_upload_options
        // changes them -- every shard of a node, every re-upload gets the same layout whatever happened to the process environment since)
        const int layout_top = opt_node_layout ? kLayoutTopLevels : 0;
        const bool planar_lights = opt_planar_lights;
        if (!build_host_image(img, s, err, env_anyhit_twin, env_anyhit_twin_dirs, layout_top, planar_lights, kTwinBudgetBytes, sphere_mode)) return fail(ATN_ERR_UNSUPPORTED, err);
        n_planar_lights = 0;
        for (const atn_light_param& l : img.lights) n_planar_lights += l._pad != 0 ? 1u : 0u;
        collect_planar_certs(s, img.lights);
        ATN_HIP(nodes.upload(img.nodes, stream));
        ATN_HIP(tris.upload(img.tris, stream));
        ATN_HIP(vtx_pos.upload(img.vtx_pos, stream));
        ATN_HIP(vtx_nml.upload(img.vtx_nml, stream));
        ATN_HIP(objects.upload(img.objects, stream));
        ATN_HIP(matrices.upload(img.matrices, stream));
        ATN_HIP(materials.upload(img.materials, stream));
        ATN_HIP(carpaint.upload(img.carpaint, stream));
        ATN_HIP(toon.upload(img.toon, stream));
        ATN_HIP(npr_lights.upload(img.npr_lights, stream));
        ATN_HIP(screen_shadow.upload(img.screen_shadow, stream));
        ATN_HIP(lights.upload(img.lights, stream));
        ATN_HIP(light_plane.upload(img.light_plane, stream));
        ATN_HIP(texels.upload(img.texels, stream));
        ATN_HIP(texels8.upload(img.texels8, stream));
        ATN_HIP(textures.upload(img.textures, stream));
        ATN_HIP(shade_tris.resize((size_t)kShadeTriQuads * (img.tris.size() ? img.tris.size() : 1)));
        if (!img.tris.empty())
            hipLaunchKernelGGL(k_pack_shade_tris, dim3(((uint32_t)img.tris.size() + 255) / 256), dim3(256), 0, stream, (const atn_triangle_param*)tris.p,
                               (const float4*)vtx_pos.p, (const float4*)vtx_nml.p, 0u, (uint32_t)img.tris.size(), shade_tris.p);
        ATN_HIP(hipGetLastError());
        ATN_HIP(hipStreamSynchronize(stream));      // `img` is pageable host memory
        scene = img.params;
        n_sphere_leaves = img.n_sphere_leaf;
        if (!env_shadow_plain) scene.shadow_plain = 0;
        scene.nodes = nodes.p; scene.tris = tris.p; scene.shade_tris = shade_tris.p; scene.vtx_pos = vtx_pos.p; scene.vtx_nml = vtx_nml.p;
        scene.objects = objects.p; scene.matrices = matrices.p; scene.materials = materials.p; scene.carpaint = carpaint.p;
        scene.toon = toon.p; scene.npr_lights = npr_lights.p; scene.screen_shadow = img.screen_shadow.empty() ? nullptr : screen_shadow.p;
        scene.lights = lights.p; scene.light_plane = light_plane.p; scene.texels = texels.p; scene.texels8 = texels8.p; scene.textures = textures.p;
        scene.mtx_quads = (uint32_t)img.matrices.size();
        has_scene = true;
        if (gm_on) { gm_sv_ids[0] = gm_sv_ids[1] = gm_rs_has_ids = false; const int grc = gm_reset_history(); if (grc) return grc; }
        src = std::move(img.source);
        light_planar.assign(img.lights.size(), 0);
        for (size_t i = 0; i < img.lights.size(); i++) light_planar[i] = img.lights[i]._pad != 0 ? 1 : 0;
        host_textures = img.textures; n_texels_used = img.texels.size();
        { const int nrc = npr_decode(img.materials); if (nrc) return nrc; }
        vl_grids.clear();       // (an upload drops the grids of atn_volume_set_grids; the material edits keep them)
        { const int vrc = vol_decode(img.materials); if (vrc) return vrc; }
        {
            const int32_t ei = s->config.bg.envmap_tex_idx;
            int orc = refresh_envmap(ei >= 0 && (uint32_t)ei < s->n_textures ? s->textures[ei].texels : nullptr);
            if (orc) return orc;
        }
        list_root_link = img.list_root_link; list_twin_delta = img.list_twin_delta; tlas_refs = img.tlas_refs;
        list_base = img.list_root; list_bytes = img.list_bytes; list_tri_leaves = img.list_tri_leaves; list_inner = img.list_inner;
        n_scene_tris = s->n_triangles; n_scene_vtx = s->n_vertices; n_scene_mtrls = s->n_materials;
        top_base = img.list_root[0];        // byte offset of the top layer's first record (the image's tail)
        n_bottom_nodes = img.n_nodes - s->bvh_lists[0].count;
        n_host_matrices = s->n_matrices;
        host_matrices.assign(s->matrices, s->matrices + s->n_matrices);     // (update_tlas without matrices still recognises identity instances)
        host_objects.assign(s->objects, s->objects + s->n_objects);
        tl.table_current = false;
        tree_is_deep = img.n_nodes >= kRefillMinNodes;
        return ATN_OK;
    }

    // Optional samplers, both OFF by default because they leave the sample stream of aten::PathTracing (the parity
    // path): the IBL light sampled from ImageBasedLight::preCompute's tables (light/ibl.cpp:10-118,180-230) and
    // texture::AtWithBilinear (image/texture.cpp:77-125) instead of texture::at for every texture lookup.
    int apply_sampling_options()
    {
        scene.tex_bilinear = opt_tex_bilinear;
        scene.ibl_importance = 0;
        scene.ibl_cdf_v = nullptr; scene.ibl_cdf_u = nullptr; scene.ibl_w = 0; scene.ibl_h = 0;
        if (!opt_ibl_importance || env_host.empty()) return ATN_OK;
        if (!ibl_tables_ready) {
            IblTables t;
            const int32_t w = env_w, h = env_h;
            const atn_vec4* tex = env_host.data();
            const float mul = env_multiplyer;
            ibl_precompute(t, w, h, [&](int32_t x, int32_t y, float& r, float& g, float& b) {
                // SampleFromUVWithTexture(u, v) = texture::at(u, v) * multiplyer at the texel centre (ibl.cpp:57-60)
                const float u = (float)(x + 0.5) / w, v = (float)(y + 0.5) / h;
                int32_t iu = (int32_t)(u * (float)(w - 1)), iv = (int32_t)(v * (float)(h - 1));
                iu = iu < 0 ? 0 : (iu > w - 1 ? w - 1 : iu); iv = iv < 0 ? 0 : (iv > h - 1 ? h - 1 : iv);
                const atn_vec4& c = tex[(size_t)iv * w + iu];
                r = c.x * mul; g = c.y * mul; b = c.z * mul;
            });
            ATN_HIP(ibl_cdf_v.upload(t.cdf_v, stream));
            ATN_HIP(ibl_cdf_u.upload(t.cdf_u, stream));
            ATN_HIP(hipStreamSynchronize(stream));
            ibl_tables_ready = true;
        }
        scene.ibl_cdf_v = ibl_cdf_v.p; scene.ibl_cdf_u = ibl_cdf_u.p; scene.ibl_w = env_w; scene.ibl_h = env_h;
        scene.ibl_importance = 1;
        return ATN_OK;
    }
    // The host copy of the environment map the config names (what the IBL tables are built from), then the sampling options again.
    // `texels`: that texture's content where the caller has just handed it in; null: read back from the device.
    int refresh_envmap(const atn_vec4* texels)
    {
        env_host.clear(); env_w = env_h = 0; ibl_tables_ready = false;
        const int32_t ei = src.config.bg.envmap_tex_idx;
        if (ei >= 0 && (size_t)ei < src.tex.size() && src.config.bg.enable_env_map) {
            const HostTexInfo& t = src.tex[ei];
            if (texels) env_host.assign(texels, texels + (size_t)t.width * t.height);
            else { const int rc = download_texture(ei, env_host); if (rc) return rc; }
            env_w = t.width; env_h = t.height; env_multiplyer = src.config.bg.multiplyer;
        }
        return apply_sampling_options();
    }
    // texture `i` as the floats a lookup returns (fetch_texel's conversions, which give back the caller's floats)
    int download_texture(int32_t i, std::vector<atn_vec4>& out)
    {
        const DevTexture& t = host_textures[i];
        const size_t n = (size_t)t.width * t.height;
        out.resize(n);
        if (!n) return ATN_OK;
        if (t.format == 0) {
            ATN_HIP(hipMemcpyAsync(out.data(), texels.p + t.offset, n * sizeof(float4), hipMemcpyDeviceToHost, stream));
            ATN_HIP(hipStreamSynchronize(stream));
            return ATN_OK;
        }
        std::vector<uint32_t> packed(n);
        ATN_HIP(hipMemcpyAsync(packed.data(), texels8.p + t.offset, n * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        ATN_HIP(hipStreamSynchronize(stream));
        const float norm = 1.0F / 255;
        for (size_t j = 0; j < n; j++) {
            const uint32_t p = packed[j];
            const float r = (float)(p & 255u), g = (float)((p >> 8) & 255u), b = (float)((p >> 16) & 255u), a = (float)(p >> 24);
            out[j] = t.format == 1 ? atn_vec4{ r / 255.0F, g / 255.0F, b / 255.0F, a / 255.0F } : atn_vec4{ r * norm, g * norm, b * norm, a * norm };
        }
        return ATN_OK;
    }

    // ---------------------------------------------------------------------------------------------------------------
    // Scene edits (docs/SCENE_EDITS.md): ≙ idaten::Renderer::updateMaterial / updateLight / UpdateTexture /
    // UpdateSceneRenderingConfig, src/libidaten/kernel/renderer.cpp:207-252.  Each call applies the change to a copy of `src`, derives
    // the device form with the functions the upload uses (host/scene_upload.hpp) and only then writes buffers and DevScene fields: a
    // refused edit leaves everything as it was.  They wait for the frames in flight and reset nothing.

    // the material-derived state of src.materials -> device
    int commit_materials(const MaterialState& ms)
    {
        ATN_HIP(materials.upload(ms.materials, stream));
        ATN_HIP(carpaint.upload(ms.carpaint, stream));
        ATN_HIP(toon.upload(ms.toon, stream));
        ATN_HIP(hipStreamSynchronize(stream));
        scene.any_alpha = ms.any_alpha; scene.material_set = ms.material_set; scene.rr_lookahead = ms.rr_lookahead;
        scene.nee_deferral = nee_deferral_class(scene.material_set, src.lights.data(), (uint32_t)src.lights.size());
        { const int rc = npr_decode(ms.materials); if (rc) return rc; }
        return vol_decode(ms.materials);
    }
    int edit_begin()
    {
        ATN_HIP(hipSetDevice(device));
        return quiesce();
    }
    int update_materials(const atn_material_param* m, uint32_t n, uint32_t first)
    {
        if (!has_scene) return fail(ATN_ERR_NO_SCENE, "atn_upload_scene has not been called");
        if (!m) return fail(ATN_ERR_INVALID_ARG, "null material array");
        if ((uint64_t)first + n > src.materials.size()) return fail(ATN_ERR_INVALID_ARG, "material range outside the uploaded scene");
        MaterialState ms;
        std::string err;
        if (!edit_materials(src, m, n, first, ms, err)) return fail(ATN_ERR_UNSUPPORTED, err);
        { const int rc = edit_begin(); if (rc) return rc; }
        return commit_materials(ms);
    }
    int update_lights(const atn_light_param* l, uint32_t n, uint32_t first, int32_t npr_target)
    {
        if (!has_scene) return fail(ATN_ERR_NO_SCENE, "atn_upload_scene has not been called");
        if (!l) return fail(ATN_ERR_INVALID_ARG, "null light array");
        const std::vector<atn_light_param>& have = npr_target ? src.npr_lights : src.lights;
        if ((uint64_t)first + n > have.size()) return fail(ATN_ERR_INVALID_ARG, "light range outside the uploaded scene");
        // The planar flag (scene_upload.hpp: planar_area_light) was derived from the vertices, which the host does not keep: a light
        // whose type and object are unchanged keeps its flag, plane and certificate, any other edited light loses them, and no edit
        // grants one.  (The flag only lets a shadow walk stop early: the films are the same with and without it.)
        std::vector<atn_light_param> dev(l, l + n);
        if (!npr_target)
            for (uint32_t k = 0; k < n; k++) {
                const atn_light_param& was = have[first + k];
                dev[k]._pad = light_planar[first + k] && l[k].type == was.type && l[k].arealight_objid == was.arealight_objid ? 1 : 0;
            }
        std::string err;
        if (!edit_lights(src, l, n, first, npr_target != 0, err)) return fail(ATN_ERR_UNSUPPORTED, err);
        { const int rc = edit_begin(); if (rc) return rc; }
        if (!n) return ATN_OK;
        if (npr_target) {
            ATN_HIP(hipMemcpyAsync(npr_lights.p + first, dev.data(), (size_t)n * sizeof(atn_light_param), hipMemcpyHostToDevice, stream));
            ATN_HIP(hipStreamSynchronize(stream));
            return ATN_OK;
        }
        const float4 no_plane = make_float4(0, 0, 0, 0);
        for (uint32_t k = 0; k < n; k++) {
            const uint32_t i = first + k;
            if (!light_planar[i] || dev[k]._pad) continue;
            ATN_HIP(hipMemcpyAsync(light_plane.p + i, &no_plane, sizeof(float4), hipMemcpyHostToDevice, stream));
            light_planar[i] = 0; n_planar_lights--;
            for (size_t c = 0; c < planar_certs.size(); c++)
                if (planar_certs[c].light == (int32_t)i) { planar_certs.erase(planar_certs.begin() + (ptrdiff_t)c); break; }
        }
        ATN_HIP(hipMemcpyAsync(lights.p + first, dev.data(), (size_t)n * sizeof(atn_light_param), hipMemcpyHostToDevice, stream));
        ATN_HIP(hipStreamSynchronize(stream));
        scene.nee_deferral = nee_deferral_class(scene.material_set, src.lights.data(), (uint32_t)src.lights.size());
        scene.shadow_plain = env_shadow_plain ? shadow_plain_class(src.lights.data(), (uint32_t)src.lights.size()) : 0;
        return ATN_OK;
    }
    int update_texture(int32_t texid, const atn_texture_desc* t)
    {
        if (!has_scene) return fail(ATN_ERR_NO_SCENE, "atn_upload_scene has not been called");
        if (!t || !t->texels) return fail(ATN_ERR_INVALID_ARG, "null texture");
        if (texid < 0 || (size_t)texid >= src.tex.size()) return fail(ATN_ERR_INVALID_ARG, "texture index outside the uploaded scene");
        MaterialState ms;
        bool rederived = false;
        std::string err;
        if (!edit_texture(src, texid, *t, ms, rederived, err)) return fail(ATN_ERR_UNSUPPORTED, err);
        { const int rc = edit_begin(); if (rc) return rc; }
        // Texel storage: a lookup returns exactly the floats handed in.  RGBA8 storage takes them if every one is what its 8-bit
        // conversion gives back (either conversion: the record names it); otherwise the texture moves to float4 storage at the end
        // of `texels` and stays there.
        const size_t n = (size_t)t->width * t->height;
        DevTexture rec = host_textures[texid];
        std::vector<uint32_t> packed;
        const int32_t fmt = rec.format ? encode_texels8(*t, packed) : 0;
        if (fmt) {
            ATN_HIP(hipMemcpyAsync(texels8.p + rec.offset, packed.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
            rec.format = fmt;
        }
        else {
            if (rec.format) {
                DevBuf<float4> grown;
                ATN_HIP(grown.resize(n_texels_used + n));
                if (n_texels_used) ATN_HIP(hipMemcpyAsync(grown.p, texels.p, n_texels_used * sizeof(float4), hipMemcpyDeviceToDevice, stream));
                ATN_HIP(hipStreamSynchronize(stream));
                texels.swap(grown);
                scene.texels = texels.p;
                rec.offset = (uint32_t)n_texels_used; rec.format = 0;
                n_texels_used += n;
            }
            ATN_HIP(hipMemcpyAsync(texels.p + rec.offset, t->texels, n * sizeof(float4), hipMemcpyHostToDevice, stream));
        }
        ATN_HIP(hipMemcpyAsync(textures.p + texid, &rec, sizeof(DevTexture), hipMemcpyHostToDevice, stream));
        ATN_HIP(hipStreamSynchronize(stream));
        host_textures[texid] = rec;
        if (rederived) { const int rc = commit_materials(ms); if (rc) return rc; }
        if (texid == src.config.bg.envmap_tex_idx && src.config.bg.enable_env_map) return refresh_envmap(t->texels);
        return ATN_OK;
    }
    int update_rendering_config(const atn_scene_rendering_config* cfg)
    {
        if (!has_scene) return fail(ATN_ERR_NO_SCENE, "atn_upload_scene has not been called");
        if (!cfg) return fail(ATN_ERR_INVALID_ARG, "null rendering config");
        const atn_background was = src.config.bg;
        std::string err;
        if (!edit_config(src, *cfg, err)) return fail(ATN_ERR_UNSUPPORTED, err);
        { const int rc = edit_begin(); if (rc) return rc; }
        apply_config(scene, src.config);
        // what the NPR and volume frames read of the config (the materials are as they were: nothing is uploaded again)
        std::memcpy(&np_cfg, src.config.feature_line, sizeof(np_cfg));
        np_alpha = vl_alpha = src.config.enable_alpha_blending != 0 && maybe_alpha;
        vl_eps_bias = src.config.epsilon_bias_for_traversing_shadow_ray_in_medium;
        const atn_background& bg = src.config.bg;
        const bool had_env = was.envmap_tex_idx >= 0 && was.enable_env_map, has_env = bg.envmap_tex_idx >= 0 && bg.enable_env_map;
        if (had_env != has_env || (has_env && (was.envmap_tex_idx != bg.envmap_tex_idx || was.multiplyer != bg.multiplyer))) return refresh_envmap(nullptr);
        return ATN_OK;
    }

    int set_sampling_options(int32_t ibl_importance, int32_t tex_bilinear)
    {
        ATN_HIP(hipSetDevice(device));
        { int q = quiesce(); if (q) return q; }
        opt_ibl_importance = ibl_importance ? 1 : 0;
        opt_tex_bilinear = tex_bilinear ? 1 : 0;
        return has_scene ? apply_sampling_options() : ATN_OK;
    }

    // A top layer of `need` float4s of node image, n_objs objects and mtx_quads matrix rows: buffers that must grow are replaced
    // behind a full stop (rare: the usual tick keeps every count); the bottom-level lists are kept, the old top layer is dropped.
    int grow_for_top_layer(size_t need, size_t n_objs, size_t mtx_quads)
    {
        if (!(need > nodes.n || n_objs > objects.n || mtx_quads > matrices.n)) return ATN_OK;
        { int q = quiesce(); if (q) return q; }
        drop_alt_set();         // re-cloned from the grown buffers at the next flip
        if (need > nodes.n) {
            float4* bigger = nullptr;
            ATN_HIP(hipMalloc((void**)&bigger, need * sizeof(float4)));
            hipError_t e = hipMemcpyAsync(bigger, nodes.p, (size_t)top_base, hipMemcpyDeviceToDevice, stream);
            if (e == hipSuccess) e = hipStreamSynchronize(stream);
            if (e != hipSuccess) { (void)hipFree(bigger); return fail(ATN_ERR_HIP, hipGetErrorString(e)); }
            nodes.release();
            nodes.p = bigger; nodes.n = need;
        }
        if (n_objs > objects.n) ATN_HIP(objects.resize(n_objs));
        if (mtx_quads > matrices.n) ATN_HIP(matrices.resize(mtx_quads));
        return ATN_OK;
    }

    // ≙ idaten::Renderer::updateBVH, src/libidaten/kernel/renderer.cpp:133-153: new object parameters and matrices
    // plus a rebuilt top layer; the bottom-level lists stay where they are in HBM.
    int updateBVH(const atn_object_param* objs, uint32_t n_objs, const atn_mat4* mtxs, uint32_t n_mtxs,
                  const atn_bvh_node* top, uint32_t n_top)
    {
        if (!has_scene) return fail(ATN_ERR_NO_SCENE, "atn_upload_scene has not been called");
        if (!objs || n_objs == 0 || !top || n_top == 0) return fail(ATN_ERR_INVALID_ARG, "empty object or top-layer array");
        ATN_HIP(hipSetDevice(device));
        if ((uint64_t)top_base + (uint64_t)n_top * kInnerBytes >= (1ull << 31)) return fail(ATN_ERR_UNSUPPORTED, "too many BVH nodes for 31-bit byte-offset links");
        if (n_mtxs && !mtxs) return fail(ATN_ERR_INVALID_ARG, "null matrix array");
        {
            std::string rerr;
            if (!validate_ranges(objs, n_objs, n_mtxs ? n_mtxs : n_host_matrices, nullptr, rerr)) return fail(ATN_ERR_UNSUPPORTED, rerr);
            for (uint32_t i = 0; i < n_objs; i++)
                if (objs[i].light_id >= scene.n_lights) return fail(ATN_ERR_UNSUPPORTED, "object light id out of range");
        }
        // the new top layer: every top-layer record is kInnerBytes long, laid out in walk order at the image's tail
        ListLayout lay;
        std::string err;
        if (!analyse_list(lay, top, n_top, true, err, SphereLeafRule{ sphere_mode, objs, n_objs })) return fail(ATN_ERR_UNSUPPORTED, err);
        for (uint32_t j = 0; j < lay.order.size(); j++) {
            if (lay.kind[j] == KIND_TRI) return fail(ATN_ERR_UNSUPPORTED, "triangle leaves in this list need a full scene upload");
            lay.offset[j] = top_base + j * kInnerBytes;
        }
        ListEmitCtx c;
        c.objects = objs; c.n_objects = n_objs; c.n_matrices = n_mtxs ? n_mtxs : n_host_matrices;
        c.matrices = n_mtxs ? mtxs : (host_matrices.size() == n_host_matrices ? host_matrices.data() : nullptr);
        c.list_root_link = list_root_link.data(); c.n_lists = (uint32_t)list_root_link.size();
        c.list_twin_delta = list_twin_delta.size() == list_root_link.size() ? list_twin_delta.data() : nullptr;
        std::vector<HostSceneImage::TlasRef> new_refs;
        c.tlas_refs = &new_refs;
        const size_t top_bytes = lay.order.size() * (size_t)kInnerBytes;
        std::vector<float4> rec(top_bytes / 16 + 1, make_float4(0, 0, 0, 0));
        int32_t root = kLinkEnd;
        uint64_t counts[3] = { 0, 0, 0 };
        if (!emit_list(reinterpret_cast<char*>(rec.data()), lay, top, c, root, counts, err, top_base)) return fail(ATN_ERR_UNSUPPORTED, err);
        if (c.n_sphere_leaf && !sphere_materials_ok(objs, n_objs, (uint32_t)scene.n_materials, err)) return fail(ATN_ERR_UNSUPPORTED, err);
        std::vector<float4> mv;
        if (n_mtxs) {
            mv.resize((size_t)n_mtxs * 4);
            for (uint32_t i = 0; i < n_mtxs; i++)
                for (int r = 0; r < 4; r++)
                    mv[4 * (size_t)i + r] = make_float4(mtxs[i].m[r][0], mtxs[i].m[r][1], mtxs[i].m[r][2], mtxs[i].m[r][3]);
        }
        const size_t need = ((size_t)top_base + top_bytes + 15) / 16;
        const size_t obj_bytes = (size_t)n_objs * sizeof(atn_object_param), mtx_bytes = mv.size() * sizeof(float4);
        // Buffers that must grow are replaced behind a full stop; otherwise the update is enqueued behind the frames in flight
        // and the host goes on.
        { int r = grow_for_top_layer(need, n_objs, mv.size()); if (r) return r; }
        { int r = begin_scene_update(top_bytes + obj_bytes + mtx_bytes + 512); if (r) return r; }
        { int r = stage_copy(reinterpret_cast<char*>(nodes.p) + top_base, rec.data(), top_bytes); if (r) return r; log_range(SB_NODES, top_base, top_bytes); }
        { int r = stage_copy(objects.p, objs, obj_bytes); if (r) return r; log_range(SB_OBJECTS, 0, obj_bytes); }
        if (n_mtxs) { int r = stage_copy(matrices.p, mv.data(), mtx_bytes); if (r) return r; log_range(SB_MATRICES, 0, mtx_bytes); n_host_matrices = n_mtxs; host_matrices.assign(mtxs, mtxs + n_mtxs); }
        { int r = end_scene_update(); if (r) return r; }
        list_root_link[0] = root;
        n_sphere_leaves = c.n_sphere_leaf;
        // a light's instance may have a new matrix, or point at another object / matrix (an objs-only update too): the flags hold only
        // if every planar light's records came back byte for byte
        if (scene.planar_lights && !planar_certs_survive_objects(objs, n_objs, mtxs, n_mtxs)) scene.planar_lights = 0;
        tlas_refs.swap(new_refs);
        if (objs != host_objects.data()) host_objects.assign(objs, objs + n_objs);
        tl.table_current = false;       // (atn_tlas_rebuild's leaf table follows the host-given top layer)
        scene.root_link = root;
        fill_root_direct(scene, rec.data(), top_base, n_mtxs ? mtxs : (host_matrices.size() == n_host_matrices ? host_matrices.data() : nullptr), n_mtxs ? n_mtxs : n_host_matrices);
        scene.node_bytes = (uint32_t)(top_base + top_bytes);
        scene.ident_row = c.ident_row;
        if (n_mtxs) scene.mtx_quads = (uint32_t)mv.size();
        point_scene_at_current_set();
        tree_is_deep = n_bottom_nodes + n_top >= kRefillMinNodes;
        return ATN_OK;
    }

    // ---------------------------------------------------------------------------------------------------------------
    // Dynamic geometry: ≙ the per-tick sequence of src/deformation_renderer/main.cpp:636-710
    //   skinning -> LBVHBuilder::build into the renderer's node list -> Renderer::updateGeometry -> Renderer::updateBVH.

    // ≙ idaten::Renderer::updateGeometry, src/libidaten/kernel/renderer.cpp:155-215: overwrite a range of the scene's
    // vertices and triangles.  (The BVH records of lists over these triangles hold hoisted vertex data: rebuild them.)
    int updateGeometry(const atn_vec4* pos, const atn_vec4* nml, uint32_t n_vtx, uint32_t vtx_offset,
                       const atn_triangle_param* tr, uint32_t n_tr, uint32_t tri_offset)
    {
        if (!has_scene) return fail(ATN_ERR_NO_SCENE, "atn_upload_scene has not been called");
        if ((n_vtx && !pos && !nml) || (n_tr && !tr)) return fail(ATN_ERR_INVALID_ARG, "null geometry array");
        if ((uint64_t)vtx_offset + n_vtx > n_scene_vtx) return fail(ATN_ERR_INVALID_ARG, "vertex range outside the uploaded scene");
        if ((uint64_t)tri_offset + n_tr > n_scene_tris) return fail(ATN_ERR_INVALID_ARG, "triangle range outside the uploaded scene");
        for (uint32_t i = 0; i < n_tr; i++) {
            if (tr[i].mtrlid >= 0 && (uint32_t)tr[i].mtrlid >= n_scene_mtrls) return fail(ATN_ERR_UNSUPPORTED, "triangle material id out of range");
            for (int v = 0; v < 3; v++)
                if (tr[i].idx[v] < 0 || (uint32_t)tr[i].idx[v] >= n_scene_vtx) return fail(ATN_ERR_UNSUPPORTED, "triangle vertex index out of range");
        }
        skins_note_triangles(tr, n_tr, tri_offset);
        ATN_HIP(hipSetDevice(device));
        // a light's vertices or triangles may be among these: then its shadow rays walk to their closest hit from here on
        if (scene.planar_lights && !planar_certs_survive_geometry(vtx_offset, n_vtx, tri_offset, n_tr)) scene.planar_lights = 0;
        const size_t vb = (size_t)n_vtx * sizeof(float4), tb = (size_t)n_tr * sizeof(atn_triangle_param);
        { int r = begin_scene_update((pos ? vb : 0) + (nml ? vb : 0) + tb + 256); if (r) return r; }
        if (n_vtx && pos) { int r = stage_copy(vtx_pos.p + vtx_offset, pos, vb); if (r) return r; log_range(SB_VTX_POS, (size_t)vtx_offset * sizeof(float4), vb); }
        if (n_vtx && nml) { int r = stage_copy(vtx_nml.p + vtx_offset, nml, vb); if (r) return r; log_range(SB_VTX_NML, (size_t)vtx_offset * sizeof(float4), vb); }
        if (n_tr) { int r = stage_copy(tris.p + tri_offset, tr, tb); if (r) return r; log_range(SB_TRIS, (size_t)tri_offset * sizeof(atn_triangle_param), tb); }
        // which triangles use the new vertices is not known here: repack every shading record (a copy of the scene arrays)
        { int r = repack_shade_tris(0, n_scene_tris); if (r) return r; }
        return end_scene_update();
    }

    int repack_shade_tris(uint32_t first, uint32_t count)
    {
        if (!count) return ATN_OK;
        hipLaunchKernelGGL(k_pack_shade_tris, dim3((count + 255) / 256), dim3(256), 0, upd, (const atn_triangle_param*)tris.p,
                           (const float4*)vtx_pos.p, (const float4*)vtx_nml.p, first, count, shade_tris.p);
        ATN_HIP(hipGetLastError());
        log_range(SB_SHADE, (size_t)first * kShadeTriQuads * sizeof(float4), (size_t)count * kShadeTriQuads * sizeof(float4));
        return ATN_OK;
    }

    int lbvh_reserve(uint32_t n)
    {
        const uint32_t rounds = radix_rounds(n), tile = kSortThreads * rounds, nb = (n + tile - 1) / tile, nn = 2 * n - 1;
        for (int k = 0; k < 2; k++) {
            if (lb.codes[k].n < n) ATN_HIP(lb.codes[k].resize(n));
            if (lb.indices[k].n < n) ATN_HIP(lb.indices[k].resize(n));
        }
        if (lb.counts.n < 256u * nb) ATN_HIP(lb.counts.resize(256u * nb));
        if (lb.totals.n < 256u) ATN_HIP(lb.totals.resize(256u));
        if (lb.arrived.n < n) ATN_HIP(lb.arrived.resize(n));
        if (lb.offs.n < nn) ATN_HIP(lb.offs.resize(nn));
        if (lb.left.n < nn) ATN_HIP(lb.left.resize(nn));
        if (lb.right.n < nn) ATN_HIP(lb.right.resize(nn));
        if (lb.parent.n < nn) ATN_HIP(lb.parent.resize(nn));
        if (lb.first.n < n) ATN_HIP(lb.first.resize(n));
        if (lb.last.n < n) ATN_HIP(lb.last.resize(n));
        if (lb.ref_nodes.n < nn) ATN_HIP(lb.ref_nodes.resize(nn));
        if (lb.pre.n < n) ATN_HIP(lb.pre.resize(n));
        if (lb.suf.n < n) ATN_HIP(lb.suf.resize(n));
        { const uint32_t ns = (n + kBoundsBlock * kBoundsSuper - 1) / (kBoundsBlock * kBoundsSuper); if (lb.sup.n < ns) ATN_HIP(lb.sup.resize(ns)); }
        return ATN_OK;
    }

    // Morton codes -> sort -> hierarchy -> links -> boxes, all enqueued on `stream`; the tree is left in lb.ref_nodes in
    // the reference's node order.  `tr` points at the first of the n triangles, `vtx` at the vertex array.
    // (box_dev: the box in device memory instead of bmin / bmax -- a skin's, atn_lbvh_rebuild_list_skinned)
    int lbvh_enqueue(const atn_triangle_param* tr, uint32_t n, int32_t tri_id_offset, const float* bmin, const float* bmax,
                     const float4* vtx, int32_t vtx_offset, uint32_t image_base, hipStream_t st, const float* box_dev = nullptr)
    {
        { int r = lbvh_reserve(n); if (r) return r; }
        const uint32_t rounds = radix_rounds(n), tile = kSortThreads * rounds, nb = (n + tile - 1) / tile, nn = 2 * n - 1;
        const dim3 b256(256);
        if (box_dev) skin_launch_morton(st, tr, vtx, vtx_offset, n, box_dev, lb.codes[0].p, lb.indices[0].p);
        else {
            f3 mn, mx;
            mn.x = bmin[0]; mn.y = bmin[1]; mn.z = bmin[2]; mx.x = bmax[0]; mx.y = bmax[1]; mx.z = bmax[2];
            hipLaunchKernelGGL(k_lbvh_morton, dim3((n + 255) / 256), b256, 0, st, tr, vtx, vtx_offset, n, mn, mx, lb.codes[0].p, lb.indices[0].p);
        }
        for (uint32_t pass = 0; pass < 4; pass++) {
            const int in = pass & 1, out = in ^ 1;
            hipLaunchKernelGGL(k_radix_count, dim3(nb), dim3(kSortThreads), 0, st, (const uint32_t*)lb.codes[in].p, n, pass * 8u, lb.counts.p, nb, rounds);
            hipLaunchKernelGGL(k_radix_scan, dim3(256), dim3(64), 0, st, lb.counts.p, nb, lb.totals.p);
            hipLaunchKernelGGL(k_radix_scatter, dim3(nb), dim3(kSortThreads), 0, st, (const uint32_t*)lb.codes[in].p, (const uint32_t*)lb.indices[in].p,
                               lb.codes[out].p, lb.indices[out].p, n, pass * 8u, (const uint32_t*)lb.counts.p, nb, (const uint32_t*)lb.totals.p, rounds);
        }
        LbvhTopo t{ lb.left.p, lb.right.p, lb.parent.p, lb.first.p, lb.last.p };
        hipLaunchKernelGGL(k_lbvh_hierarchy, dim3((n + 255) / 256), b256, 0, st, (const uint32_t*)lb.codes[0].p, n, t, lb.arrived.p);
        hipLaunchKernelGGL(k_lbvh_links, dim3((nn + 255) / 256), b256, 0, st, n, tri_id_offset, t, (const uint32_t*)lb.indices[0].p, lb.ref_nodes.p,
                           image_base, lb.offs.p);
        {
            const uint32_t nblk = (n + kBoundsBlock - 1) / kBoundsBlock, nsup = (nblk + kBoundsSuper - 1) / kBoundsSuper;
            hipLaunchKernelGGL(k_lbvh_bounds_block, dim3(nblk), dim3(kBoundsBlock), 0, st, n, t, (const uint32_t*)lb.indices[0].p, tr, vtx, vtx_offset,
                               lb.ref_nodes.p, lb.arrived.p, lb.pre.p, lb.suf.p);
            hipLaunchKernelGGL(k_lbvh_bounds_super, dim3(nsup), dim3(64), 0, st, n, (const LbvhBox*)lb.pre.p, lb.sup.p);
            hipLaunchKernelGGL(k_lbvh_bounds_cross, dim3((n + 255) / 256), b256, 0, st, n, t, (const LbvhBox*)lb.pre.p, (const LbvhBox*)lb.suf.p,
                               (const LbvhBox*)lb.sup.p, lb.ref_nodes.p);
        }
        ATN_HIP(hipGetLastError());
        return ATN_OK;
    }

    // ≙ idaten::LBVHBuilder::build(dst, std::vector<TriangleParameter>&, ..., threadedBvhNodes), LBVHBuilder.cu:812-833:
    // host arrays in, the ThreadedBvhNode array out, in the reference's node order.
    int lbvh_build(const atn_triangle_param* tr, uint32_t n, int32_t tri_id_offset, const float* bmin, const float* bmax,
                   const atn_vec4* vtx, uint32_t n_vtx, int32_t vtx_offset, atn_bvh_node* out, uint32_t* out_codes, uint32_t* out_indices)
    {
        if (!tr || !vtx || !out || !bmin || !bmax) return fail(ATN_ERR_INVALID_ARG, "null argument");
        if (n < 2) return fail(ATN_ERR_INVALID_ARG, "an LBVH needs at least two triangles");
        if (n > kLbvhMaxTris) return fail(ATN_ERR_UNSUPPORTED, "too many triangles: node indices are stored as floats");
        for (uint32_t i = 0; i < n; i++)
            for (int v = 0; v < 3; v++) {
                const int64_t j = (int64_t)tr[i].idx[v] + vtx_offset;
                if (j < 0 || j >= (int64_t)n_vtx) return fail(ATN_ERR_INVALID_ARG, "triangle vertex index out of range");
            }
        ATN_HIP(hipSetDevice(device));
        ATN_HIP(hipStreamSynchronize(stream));
        if (lb.tris.n < n) ATN_HIP(lb.tris.resize(n));
        if (lb.vtx.n < n_vtx) ATN_HIP(lb.vtx.resize(n_vtx));
        ATN_HIP(hipMemcpyAsync(lb.tris.p, tr, (size_t)n * sizeof(atn_triangle_param), hipMemcpyHostToDevice, stream));
        ATN_HIP(hipMemcpyAsync(lb.vtx.p, vtx, (size_t)n_vtx * sizeof(float4), hipMemcpyHostToDevice, stream));
        { int r = lbvh_enqueue(lb.tris.p, n, tri_id_offset, bmin, bmax, lb.vtx.p, vtx_offset, 0, stream); if (r) return r; }
        ATN_HIP(hipMemcpyAsync(out, lb.ref_nodes.p, (size_t)(2 * n - 1) * sizeof(atn_bvh_node), hipMemcpyDeviceToHost, stream));
        if (out_codes) ATN_HIP(hipMemcpyAsync(out_codes, lb.codes[0].p, (size_t)n * 4, hipMemcpyDeviceToHost, stream));
        if (out_indices) ATN_HIP(hipMemcpyAsync(out_indices, lb.indices[0].p, (size_t)n * 4, hipMemcpyDeviceToHost, stream));
        ATN_HIP(hipStreamSynchronize(stream));
        return ATN_OK;
    }

    // ≙ lbvh_.build(nodes[deformPos], tris, tri_offset_, sceneBbox, vtxPos, ...) of deformation_renderer/main.cpp:686-693:
    // rebuild bottom-level list `list` as an LBVH over the scene's triangles [tri_offset, tri_offset + n) as they are on
    // the device NOW, and write its records over the list's region of the node image.  The region keeps its size: an
    // LBVH over n triangles is n - 1 inner records and n triangle leaves, so the list must have been uploaded with one
    // leaf per triangle (any full binary tree over the n triangles, e.g. atns_build_blas's).
    int lbvh_rebuild_list(uint32_t list, uint32_t tri_offset, uint32_t n, const float* bmin, const float* bmax, bool sync, const float* box_dev = nullptr)
    {
        if (!has_scene) return fail(ATN_ERR_NO_SCENE, "atn_upload_scene has not been called");
        if (!box_dev && (!bmin || !bmax)) return fail(ATN_ERR_INVALID_ARG, "null bounding box");
        if (list == 0 || list >= list_base.size()) return fail(ATN_ERR_INVALID_ARG, "not a bottom-level BVH list");
        if (n < 2) return fail(ATN_ERR_INVALID_ARG, "an LBVH needs at least two triangles");
        if (n > kLbvhMaxTris) return fail(ATN_ERR_UNSUPPORTED, "too many triangles: node indices are stored as floats");
        if ((uint64_t)tri_offset + n > n_scene_tris) return fail(ATN_ERR_INVALID_ARG, "triangle range outside the uploaded scene");
        if (list_tri_leaves[list] != n || list_inner[list] != n - 1 || list_bytes[list] != (n - 1) * kInnerBytes + n * kTriLeafBytes)
            return fail(ATN_ERR_UNSUPPORTED, "the list was not uploaded as a binary tree with one leaf per triangle of this range");
        ATN_HIP(hipSetDevice(device));
        // The list's any-hit twins (scene_upload.hpp) are threadings of the tree that is about to be replaced: they are re-threaded on
        // the device from the new tree (lbvh.hpp, k_lbvh_twin_*), into the region the upload gave them; the TLAS leaves' twin words stay.
        const int32_t twin_word = list < list_twin_delta.size() ? list_twin_delta[list] : 0;
        const uint32_t twin_delta = (uint32_t)(twin_word & ~15), twin_dirs = twin_word == 0 ? 0u : ((twin_word & 1) ? 8u : 1u);
        if (twin_word != 0 && twin_delta != list_bytes[list]) return fail(ATN_ERR_UNSUPPORTED, "the list's twins do not lie at the list's own size apart");
        { int r = begin_scene_update(64); if (r) return r; }
        // a caller may have written the scene arrays in place (atn_scene_device_arrays): refresh this mesh's shading records
        // (a skin's compute has written them already)
        if (!box_dev) { int r = repack_shade_tris(tri_offset, n); if (r) return r; }
        { int r = lbvh_enqueue(tris.p + tri_offset, n, (int32_t)tri_offset, bmin, bmax, vtx_pos.p, 0, list_base[list], upd, box_dev); if (r) return r; }
        const uint32_t nn = 2 * n - 1;
        hipLaunchKernelGGL(k_lbvh_emit, dim3((nn + 255) / 256), dim3(256), 0, upd, n, (const atn_bvh_node*)lb.ref_nodes.p, (const uint32_t*)lb.offs.p,
                           (const atn_triangle_param*)tris.p, (const float4*)vtx_pos.p, nodes.p);
        ATN_HIP(hipGetLastError());
        log_range(SB_NODES, list_base[list], list_bytes[list]);
        if (twin_dirs) {
            if (lb.flips.n < n) ATN_HIP(lb.flips.resize(n));
            LbvhTopo t{ lb.left.p, lb.right.p, lb.parent.p, lb.first.p, lb.last.p };
            hipLaunchKernelGGL(k_lbvh_twin_flips, dim3((n + 255) / 256), dim3(256), 0, upd, n, t, (const atn_bvh_node*)lb.ref_nodes.p, twin_dirs, lb.flips.p);
            hipLaunchKernelGGL(k_lbvh_twin_emit, dim3((nn + 255) / 256, twin_dirs), dim3(256), 0, upd, n, t, (const atn_bvh_node*)lb.ref_nodes.p,
                               (const uint32_t*)lb.offs.p, (const uint8_t*)lb.flips.p, twin_delta, (const atn_triangle_param*)tris.p, (const float4*)vtx_pos.p, nodes.p);
            ATN_HIP(hipGetLastError());
            log_range(SB_NODES, list_base[list] + twin_delta, (size_t)twin_dirs * twin_delta);
        }
        // the root is node 0 = an inner record at the start of the region: the TLAS leaves' root link (and twin word) stay valid
        { int r = end_scene_update(); if (r) return r; }
        if (sync) ATN_HIP(hipStreamSynchronize(upd));
        return ATN_OK;
    }

    // ---------------------------------------------------------------------------------------------------------------
    // The top layer rebuilt on the device (device/tlas.hpp, docs/TLAS.md): an LBVH over the instances' world boxes, enqueued behind
    // the frames in flight like updateBVH -- no host tree, no host wait, nothing read back.  The leaves are the KIND_TLAS leaves of
    // the last host-given top layer (tlas_refs, in that layer's walk order: the order that breaks ties between equal Morton codes).
    struct TlasScratch {
        DevBuf<TlasLeaf> table;
        DevBuf<TlasBox> wbox, partial, ubox, nbox;      // the general path's
        bool table_current = false;                     // `table` holds tlas_refs as they are (upload and updateBVH replace them)
    } tl;

    int tlas_rebuild(const atn_object_param* objs, uint32_t n_objs, const atn_mat4* mtxs, uint32_t n_mtxs, uint32_t flags)
    {
        if (!has_scene) return fail(ATN_ERR_NO_SCENE, "atn_upload_scene has not been called");
        if ((objs == nullptr) != (n_objs == 0)) return fail(ATN_ERR_INVALID_ARG, "object array and count do not match");
        if (n_mtxs && !mtxs) return fail(ATN_ERR_INVALID_ARG, "null matrix array");
        { const int sr = sph_refuse("atn_tlas_rebuild builds the top layer over instance leaves and would drop the sphere leaves"); if (sr) return sr; }
        ATN_HIP(hipSetDevice(device));
        const atn_object_param* O = objs ? objs : host_objects.data();
        const uint32_t n_o = objs ? n_objs : (uint32_t)host_objects.size();
        const uint32_t n_m = n_mtxs ? n_mtxs : n_host_matrices;
        const atn_mat4* M = n_mtxs ? mtxs : (host_matrices.size() == n_host_matrices ? host_matrices.data() : nullptr);
        // every index a kernel uses is checked here first
        {
            std::string rerr;
            if (!validate_ranges(O, n_o, n_m, nullptr, rerr)) return fail(ATN_ERR_UNSUPPORTED, rerr);
            for (uint32_t i = 0; i < n_o; i++)
                if (O[i].light_id >= scene.n_lights) return fail(ATN_ERR_UNSUPPORTED, "object light id out of range");
        }
        const size_t n_leaves = tlas_refs.size();
        if (n_leaves == 0) return fail(ATN_ERR_UNSUPPORTED, "the top layer has no instance leaf to rebuild it over");
        if (n_leaves > kLbvhMaxTris) return fail(ATN_ERR_UNSUPPORTED, "too many instances: node indices are stored as floats");
        const uint32_t n = (uint32_t)n_leaves;
        for (const HostSceneImage::TlasRef& t : tlas_refs) {
            if (t.objid < 0 || (uint32_t)t.objid >= n_o) return fail(ATN_ERR_UNSUPPORTED, "TLAS leaf object id out of range");
            if (t.list == 0 || t.list >= list_root_link.size() || list_root_link[t.list] == kLinkEnd) return fail(ATN_ERR_UNSUPPORTED, "TLAS leaf references a missing BLAS list");
        }
        const size_t top_bytes = (size_t)(2 * (uint64_t)n - 1) * kInnerBytes;
        if ((uint64_t)top_base + top_bytes >= (1ull << 31)) return fail(ATN_ERR_UNSUPPORTED, "too many BVH nodes for 31-bit byte-offset links");
        if (n == 1) {
            // fill_root_direct needs the record itself: one instance is written from the host, as updateBVH does it
            const HostSceneImage::TlasRef t = tlas_refs[0];
            atn_bvh_node top{};
            top.hit = -1.0F; top.miss = -1.0F; top.f0 = (float)t.objid; top.f1 = -1.0F; top.f3 = (float)t.meshid;
            { const uint32_t exid = t.list; std::memcpy(&top.f2, &exid, 4); }      // (the exid bit-field: mainExid = the list)
            const std::vector<atn_object_param> keep(O, O + n_o);
            return updateBVH(keep.data(), n_o, mtxs, n_mtxs, &top, 1);
        }
        std::vector<float4> mv;
        if (n_mtxs) {
            mv.resize((size_t)n_mtxs * 4);
            for (uint32_t i = 0; i < n_mtxs; i++)
                for (int r = 0; r < 4; r++)
                    mv[4 * (size_t)i + r] = make_float4(mtxs[i].m[r][0], mtxs[i].m[r][1], mtxs[i].m[r][2], mtxs[i].m[r][3]);
        }
        const size_t need = ((size_t)top_base + top_bytes + 15) / 16;
        const size_t obj_bytes = (size_t)n_objs * sizeof(atn_object_param), mtx_bytes = mv.size() * sizeof(float4);
        { int r = grow_for_top_layer(need, n_objs, mv.size()); if (r) return r; }
        const TlasLaunch l = tlas_launch(n, kTlasBlockMax, (flags & 1u) != 0);
        // Scratch.  The sort's and the hierarchy's buffers are the list rebuilds' (lb): a list rebuild of this tick is enqueued on
        // the same update stream in front of this call, and stream order is all that keeps the two apart -- nothing here may move
        // to another stream without a dependency on it.
        if (tl.table.n < n) { ATN_HIP(tl.table.resize(n)); tl.table_current = false; }
        if (!l.block_path) {
            { int r = lbvh_reserve(n); if (r) return r; }
            if (tl.wbox.n < n) ATN_HIP(tl.wbox.resize(n));
            if (tl.partial.n < l.leaf_grid) ATN_HIP(tl.partial.resize(l.leaf_grid));
            if (tl.ubox.n < 1) ATN_HIP(tl.ubox.resize(1));
            if (tl.nbox.n < 2 * (size_t)n - 1) ATN_HIP(tl.nbox.resize(2 * (size_t)n - 1));
        }
        const size_t table_bytes = tl.table_current ? 0 : (size_t)n * sizeof(TlasLeaf);
        { int r = begin_scene_update(table_bytes + obj_bytes + mtx_bytes + 512); if (r) return r; }
        if (!tl.table_current) {
            std::vector<TlasLeaf> tab(n);
            for (uint32_t k = 0; k < n; k++) {
                const HostSceneImage::TlasRef& t = tlas_refs[k];
                tab[k] = TlasLeaf{ t.objid, list_root_link[t.list], t.list < list_twin_delta.size() ? list_twin_delta[t.list] : 0, t.meshid };
            }
            { int r = stage_copy(tl.table.p, tab.data(), table_bytes); if (r) return r; }
            tl.table_current = true;
        }
        if (objs) { int r = stage_copy(objects.p, objs, obj_bytes); if (r) return r; log_range(SB_OBJECTS, 0, obj_bytes); }
        if (n_mtxs) { int r = stage_copy(matrices.p, mv.data(), mtx_bytes); if (r) return r; log_range(SB_MATRICES, 0, mtx_bytes); }
        TlasArgs a{};
        a.table = tl.table.p; a.n = n; a.top_base = top_base; a.image = nodes.p;
        a.objects = objects.p; a.matrices = matrices.p; a.tris = tris.p; a.vtx_pos = vtx_pos.p;
        a.recognise_identity = M ? 1 : 0;
        if (l.block_path) tlas_launch_block(l, upd, a);
        else {
            a.wbox = tl.wbox.p; a.partial = tl.partial.p; a.ubox = tl.ubox.p; a.nbox = tl.nbox.p; a.n_partial = l.leaf_grid;
            a.codes = lb.codes[0].p; a.indices = lb.indices[0].p; a.arrived = lb.arrived.p;
            a.topo = LbvhTopo{ lb.left.p, lb.right.p, lb.parent.p, lb.first.p, lb.last.p };
            tlas_launch_codes(l, upd, a);
            const uint32_t rounds = radix_rounds(n), tile = kSortThreads * rounds, nb = (n + tile - 1) / tile;
            for (uint32_t pass = 0; pass < 4; pass++) {     // (four passes: the sorted keys end in codes[0] / indices[0])
                const int in = pass & 1, out = in ^ 1;
                hipLaunchKernelGGL(k_radix_count, dim3(nb), dim3(kSortThreads), 0, upd, (const uint32_t*)lb.codes[in].p, n, pass * 8u, lb.counts.p, nb, rounds);
                hipLaunchKernelGGL(k_radix_scan, dim3(256), dim3(64), 0, upd, lb.counts.p, nb, lb.totals.p);
                hipLaunchKernelGGL(k_radix_scatter, dim3(nb), dim3(kSortThreads), 0, upd, (const uint32_t*)lb.codes[in].p, (const uint32_t*)lb.indices[in].p,
                                   lb.codes[out].p, lb.indices[out].p, n, pass * 8u, (const uint32_t*)lb.counts.p, nb, (const uint32_t*)lb.totals.p, rounds);
            }
            hipLaunchKernelGGL(k_lbvh_hierarchy, dim3(l.leaf_grid), dim3(256), 0, upd, (const uint32_t*)lb.codes[0].p, n, a.topo, lb.arrived.p);
            tlas_launch_emit(l, upd, a);
        }
        ATN_HIP(hipGetLastError());
        log_range(SB_NODES, top_base, top_bytes);
        { int r = end_scene_update(); if (r) return r; }
        // the host state updateBVH leaves behind
        if (n_mtxs) { n_host_matrices = n_mtxs; host_matrices.assign(mtxs, mtxs + n_mtxs); }
        if (objs) host_objects.assign(objs, objs + n_objs);
        const int32_t root = (int32_t)top_base;     // inner node 0 lies first
        list_root_link[0] = root;
        if (scene.planar_lights && !planar_certs_survive_objects(host_objects.data(), (uint32_t)host_objects.size(), mtxs, n_mtxs)) scene.planar_lights = 0;
        int32_t ident_row = -1;
        for (uint32_t k = 0; k < n; k++) {
            tlas_refs[k].offset = top_base + kInnerBytes * (n - 1 + k);
            const int32_t mtx_id = host_objects[tlas_refs[k].objid].mtx_id;
            if (ident_row < 0 && mtx_id >= 0 && M && is_exact_identity(host_matrices[(size_t)mtx_id + 1])) ident_row = 4 * (mtx_id + 1);
        }
        scene.root_link = root;
        fill_root_direct(scene, nullptr, 0);        // (an inner root: no direct entry)
        scene.node_bytes = (uint32_t)(top_base + top_bytes);
        scene.ident_row = ident_row;
        if (n_mtxs) scene.mtx_quads = (uint32_t)mv.size();
        point_scene_at_current_set();
        tree_is_deep = n_bottom_nodes + (2 * (uint64_t)n - 1) >= kRefillMinNodes;
        return ATN_OK;
    }

    // Probe: the top layer's records as they are in device memory (waits for everything)
    int tlas_download(void* out, uint32_t cap_bytes, uint32_t* out_records, int32_t* out_root_link, uint32_t* out_top_base)
    {
        if (!has_scene) return fail(ATN_ERR_NO_SCENE, "atn_upload_scene has not been called");
        ATN_HIP(hipSetDevice(device));
        { int q = quiesce(); if (q) return q; }
        const uint32_t bytes = scene.node_bytes - top_base;
        if (out_records) *out_records = bytes / kInnerBytes;
        if (out_root_link) *out_root_link = scene.root_link;
        if (out_top_base) *out_top_base = top_base;
        if (!out) return ATN_OK;
        if (cap_bytes < bytes) return fail(ATN_ERR_INVALID_ARG, "atn_tlas_download: the buffer is smaller than the top layer");
        ATN_HIP(hipMemcpyAsync(out, reinterpret_cast<const char*>(nodes.p) + top_base, bytes, hipMemcpyDeviceToHost, stream));
        ATN_HIP(hipStreamSynchronize(stream));
        return ATN_OK;
    }

    // ---------------------------------------------------------------------------------------------------------------
    // Skinning on the device (device/skinning.hpp, docs/SKINNING.md): ≙ idaten::Skinning, src/libidaten/kernel/Skinning.cu:147-375.
    struct Skin {
        uint32_t handle = 0, n_vtx = 0, vtx_off = 0, tri_off = 0, n_tri = 0, n_mtx = 0;
        bool has_palette = false, computed = false, stale = false;
        DevBuf<atn_skinning_vertex> verts;
        DevBuf<float4> palette, prev;
        DevBuf<uint32_t> partial;       // per block of the vertex pass: the block's box as keys
        DevBuf<float> box;              // min xyz, max xyz
    };
    std::vector<std::unique_ptr<Skin>> skins;
    uint32_t skin_counter = 0;          // handles are never reused: a dead handle stays dead
    Skin* find_skin(atn_skin h)
    {
        for (auto& k : skins) if (k->handle == h && h != 0) return k.get();
        return nullptr;
    }
    // an atn_update_geometry that rewrites a skin's triangles: the skin computes on only while they still name its own vertices
    void skins_note_triangles(const atn_triangle_param* tr, uint32_t n_tr, uint32_t tri_offset)
    {
        for (auto& k : skins) {
            const uint64_t lo = std::max<uint64_t>(tri_offset, k->tri_off), hi = std::min<uint64_t>((uint64_t)tri_offset + n_tr, (uint64_t)k->tri_off + k->n_tri);
            for (uint64_t t = lo; t < hi; t++)
                for (int v = 0; v < 3; v++) {
                    const int64_t j = (int64_t)tr[t - tri_offset].idx[v] - (int64_t)k->vtx_off;
                    if (j < 0 || j >= (int64_t)k->n_vtx) k->stale = true;
                }
        }
    }

    int skin_create(const atn_skinning_vertex* v, uint32_t n_vtx, uint32_t vtx_off, uint32_t tri_off, uint32_t n_tr, uint32_t n_mtx, atn_skin* out)
    {
        if (!out) return fail(ATN_ERR_INVALID_ARG, "null skin handle");
        *out = 0;
        if (!has_scene) return fail(ATN_ERR_NO_SCENE, "atn_upload_scene has not been called");
        if (scene_in_place) return fail(ATN_ERR_UNSUPPORTED, "skins are not supported once the caller writes the scene arrays itself (atn_scene_device_arrays)");
        if (!v || n_vtx == 0) return fail(ATN_ERR_INVALID_ARG, "empty skinning vertex array");
        if (n_mtx == 0) return fail(ATN_ERR_INVALID_ARG, "a skin needs at least one matrix");
        if (n_mtx > kSkinMaxMatrices) return fail(ATN_ERR_UNSUPPORTED, "too many matrices in the skin's palette");
        if ((uint64_t)vtx_off + n_vtx > n_scene_vtx) return fail(ATN_ERR_INVALID_ARG, "vertex range outside the uploaded scene");
        if ((uint64_t)tri_off + n_tr > n_scene_tris) return fail(ATN_ERR_INVALID_ARG, "triangle range outside the uploaded scene");
        for (uint32_t i = 0; i < n_vtx; i++)
            for (int k = 0; k < 4; k++) {
                const float f = v[i].blend_index[k];
                // (int)f in [0, n_mtx); a NaN fails the first comparison
                if (!(f > -1.0F && f < (float)n_mtx)) return fail(ATN_ERR_UNSUPPORTED, "blend index " + std::to_string(k) + " of vertex " + std::to_string(i) + " is outside the palette");
            }
        ATN_HIP(hipSetDevice(device));
        { int q = quiesce(); if (q) return q; }
        // the triangles as they are on the device now (the host keeps no copy)
        std::vector<atn_triangle_param> tr(n_tr);
        if (n_tr) {
            ATN_HIP(hipMemcpyAsync(tr.data(), tris.p + tri_off, (size_t)n_tr * sizeof(atn_triangle_param), hipMemcpyDeviceToHost, stream));
            ATN_HIP(hipStreamSynchronize(stream));
        }
        for (uint32_t t = 0; t < n_tr; t++)
            for (int k = 0; k < 3; k++) {
                const int64_t j = (int64_t)tr[t].idx[k] - (int64_t)vtx_off;
                if (j < 0 || j >= (int64_t)n_vtx) return fail(ATN_ERR_INVALID_ARG, "triangle " + std::to_string(tri_off + t) + " names a vertex outside the skin's vertex range");
            }
        std::unique_ptr<Skin> k(new Skin());
        k->n_vtx = n_vtx; k->vtx_off = vtx_off; k->tri_off = tri_off; k->n_tri = n_tr; k->n_mtx = n_mtx;
        const SkinLaunch l = skin_launch(n_vtx, n_tr, n_mtx, kSkinPaletteLds);
        ATN_HIP(k->verts.resize(n_vtx)); ATN_HIP(k->palette.resize(4u * (size_t)n_mtx)); ATN_HIP(k->prev.resize(n_vtx));
        ATN_HIP(k->partial.resize(6u * (size_t)l.vtx_grid)); ATN_HIP(k->box.resize(6));
        ATN_HIP(hipMemcpyAsync(k->verts.p, v, (size_t)n_vtx * sizeof(atn_skinning_vertex), hipMemcpyHostToDevice, stream));
        ATN_HIP(hipMemsetAsync(k->prev.p, 0, (size_t)n_vtx * sizeof(float4), stream));
        ATN_HIP(hipMemsetAsync(k->box.p, 0, 6 * sizeof(float), stream));
        ATN_HIP(hipStreamSynchronize(stream));      // `v` is pageable host memory
        k->handle = ++skin_counter;
        *out = k->handle;
        skins.push_back(std::move(k));
        return ATN_OK;
    }

    int skin_destroy(atn_skin h)
    {
        if (!find_skin(h)) return fail(ATN_ERR_INVALID_ARG, "not a live skin (destroyed, or older than the last atn_upload_scene)");
        ATN_HIP(hipSetDevice(device));
        { int q = quiesce(); if (q) return q; }     // its buffers may be in use on the update stream
        for (size_t i = 0; i < skins.size(); i++) if (skins[i]->handle == h) { skins.erase(skins.begin() + (long)i); break; }
        return ATN_OK;
    }

    // ≙ Skinning::update, Skinning.cu:214-225
    int skin_update(atn_skin h, const atn_mat4* m, uint32_t n)
    {
        Skin* k = find_skin(h);
        if (!k) return fail(ATN_ERR_INVALID_ARG, "not a live skin (destroyed, or older than the last atn_upload_scene)");
        if (!m) return fail(ATN_ERR_INVALID_ARG, "null matrix array");
        if (n != k->n_mtx) return fail(ATN_ERR_INVALID_ARG, "the palette must hold the skin's " + std::to_string(k->n_mtx) + " matrices");
        ATN_HIP(hipSetDevice(device));
        const size_t bytes = (size_t)n * sizeof(atn_mat4);
        { int r = begin_scene_update(bytes + 256); if (r) return r; }
        { int r = stage_copy(k->palette.p, m, bytes); if (r) return r; }      // atn_mat4 is four float4 rows
        { int r = end_scene_update(); if (r) return r; }
        k->has_palette = true;
        return ATN_OK;
    }

    // ≙ Skinning::compute, Skinning.cu:227-345
    int skin_compute(atn_skin h, bool restart, float* bmin, float* bmax)
    {
        Skin* k = find_skin(h);
        if (!k) return fail(ATN_ERR_INVALID_ARG, "not a live skin (destroyed, or older than the last atn_upload_scene)");
        if ((bmin == nullptr) != (bmax == nullptr)) return fail(ATN_ERR_INVALID_ARG, "give both corners of the box or neither");
        if (!k->has_palette) return fail(ATN_ERR_INVALID_ARG, "atn_skin_update has not been called on this skin");
        if (scene_in_place) return fail(ATN_ERR_UNSUPPORTED, "skins are not supported once the caller writes the scene arrays itself (atn_scene_device_arrays)");
        if (k->stale) return fail(ATN_ERR_UNSUPPORTED, "atn_update_geometry rewrote the skin's triangles with vertices outside the skin's range");
        ATN_HIP(hipSetDevice(device));
        // the lamp's vertices or triangles may be among these (updateGeometry's rule)
        if (scene.planar_lights && !planar_certs_survive_geometry(k->vtx_off, k->n_vtx, k->tri_off, k->n_tri)) scene.planar_lights = 0;
        { int r = begin_scene_update(64); if (r) return r; }
        const SkinLaunch l = skin_launch(k->n_vtx, k->n_tri, k->n_mtx, kSkinPaletteLds);
        SkinVtxArgs va{};
        va.verts = reinterpret_cast<const uint2*>(k->verts.p); va.palette = k->palette.p;
        va.pos = vtx_pos.p + k->vtx_off; va.nml = vtx_nml.p + k->vtx_off; va.prev = k->prev.p; va.partial = k->partial.p;
        va.n_vtx = k->n_vtx; va.n_mtx = k->n_mtx; va.restart = restart ? 1 : 0;
        skin_launch_vertices(l, upd, va);
        SkinTriArgs ta{};
        ta.tris = tris.p; ta.vtx_pos = vtx_pos.p; ta.vtx_nml = vtx_nml.p; ta.shade_tris = shade_tris.p;
        ta.first = k->tri_off; ta.count = k->n_tri; ta.partial = k->partial.p; ta.n_partial = l.vtx_grid; ta.box = k->box.p;
        skin_launch_triangles(l, upd, ta);
        ATN_HIP(hipGetLastError());
        const size_t vb = (size_t)k->n_vtx * sizeof(float4);
        log_range(SB_VTX_POS, (size_t)k->vtx_off * sizeof(float4), vb);
        log_range(SB_VTX_NML, (size_t)k->vtx_off * sizeof(float4), vb);
        log_range(SB_TRIS, (size_t)k->tri_off * sizeof(atn_triangle_param), (size_t)k->n_tri * sizeof(atn_triangle_param));
        log_range(SB_SHADE, (size_t)k->tri_off * kShadeTriQuads * sizeof(float4), (size_t)k->n_tri * kShadeTriQuads * sizeof(float4));
        { int r = end_scene_update(); if (r) return r; }
        k->computed = true;
        if (bmin) {
            float b[6];
            ATN_HIP(hipMemcpyAsync(b, k->box.p, sizeof(b), hipMemcpyDeviceToHost, upd));
            ATN_HIP(hipStreamSynchronize(upd));
            for (int c = 0; c < 3; c++) { bmin[c] = b[c]; bmax[c] = b[3 + c]; }
        }
        return ATN_OK;
    }

    int lbvh_rebuild_list_skinned(uint32_t list, atn_skin h)
    {
        Skin* k = find_skin(h);
        if (!k) return fail(ATN_ERR_INVALID_ARG, "not a live skin (destroyed, or older than the last atn_upload_scene)");
        if (!k->computed) return fail(ATN_ERR_INVALID_ARG, "atn_skin_compute has not been called on this skin: there is no box yet");
        if (scene_in_place) return fail(ATN_ERR_UNSUPPORTED, "skins are not supported once the caller writes the scene arrays itself (atn_scene_device_arrays)");
        return lbvh_rebuild_list(list, k->tri_off, k->n_tri, nullptr, nullptr, false, k->box.p);
    }

    int skin_download(atn_skin h, int32_t which, void* out)
    {
        Skin* k = find_skin(h);
        if (!k) return fail(ATN_ERR_INVALID_ARG, "not a live skin (destroyed, or older than the last atn_upload_scene)");
        if (!out || which < 0 || which > 8) return fail(ATN_ERR_INVALID_ARG, "atn_skin_download: null output or unknown buffer");
        ATN_HIP(hipSetDevice(device));
        { int q = quiesce(); if (q) return q; }
        const size_t vb = (size_t)k->n_vtx * sizeof(float4);
        if (which == 0) ATN_HIP(hipMemcpyAsync(out, vtx_pos.p + k->vtx_off, vb, hipMemcpyDeviceToHost, stream));
        else if (which == 1) ATN_HIP(hipMemcpyAsync(out, vtx_nml.p + k->vtx_off, vb, hipMemcpyDeviceToHost, stream));
        else if (which == 2) ATN_HIP(hipMemcpyAsync(out, k->prev.p, vb, hipMemcpyDeviceToHost, stream));
        else if (which == 3) ATN_HIP(hipMemcpyAsync(out, k->box.p, 6 * sizeof(float), hipMemcpyDeviceToHost, stream));
        // the WHOLE scene as new frames read it: what a tick must leave alone outside the skin's ranges
        else if (which == 5) ATN_HIP(hipMemcpyAsync(out, shade_tris.p, (size_t)n_scene_tris * kShadeTriQuads * sizeof(float4), hipMemcpyDeviceToHost, stream));
        else if (which == 6) ATN_HIP(hipMemcpyAsync(out, vtx_pos.p, (size_t)n_scene_vtx * sizeof(float4), hipMemcpyDeviceToHost, stream));
        else if (which == 7) ATN_HIP(hipMemcpyAsync(out, vtx_nml.p, (size_t)n_scene_vtx * sizeof(float4), hipMemcpyDeviceToHost, stream));
        else if (which == 8) ATN_HIP(hipMemcpyAsync(out, tris.p, (size_t)n_scene_tris * sizeof(atn_triangle_param), hipMemcpyDeviceToHost, stream));
        else {
            std::vector<atn_triangle_param> tr(k->n_tri);
            if (k->n_tri) ATN_HIP(hipMemcpyAsync(tr.data(), tris.p + k->tri_off, (size_t)k->n_tri * sizeof(atn_triangle_param), hipMemcpyDeviceToHost, stream));
            ATN_HIP(hipStreamSynchronize(stream));
            for (uint32_t t = 0; t < k->n_tri; t++) static_cast<float*>(out)[t] = tr[t].area;
        }
        ATN_HIP(hipStreamSynchronize(stream));
        return ATN_OK;
    }

    int download_list(uint32_t list, void* out, uint32_t capacity, uint32_t* n_bytes)
    {
        if (!has_scene) return fail(ATN_ERR_NO_SCENE, "atn_upload_scene has not been called");
        if (list == 0 || list >= list_base.size()) return fail(ATN_ERR_INVALID_ARG, "not a bottom-level BVH list");
        const int32_t twin_word = list < list_twin_delta.size() ? list_twin_delta[list] : 0;
        const uint32_t twin_delta = (uint32_t)(twin_word & ~15), twin_dirs = twin_word == 0 ? 0u : ((twin_word & 1) ? 8u : 1u);
        const uint64_t bytes = twin_dirs ? (uint64_t)twin_delta * (1u + twin_dirs) : list_bytes[list];
        if ((uint64_t)list_base[list] + bytes > nodes.n * sizeof(float4)) return fail(ATN_ERR_UNSUPPORTED, "the list's region leaves the node image (internal)");
        if (n_bytes) *n_bytes = (uint32_t)bytes;
        if (!out) return ATN_OK;
        if (capacity < bytes) return fail(ATN_ERR_INVALID_ARG, "output buffer too small for the list");
        ATN_HIP(hipSetDevice(device));
        { int q = quiesce(); if (q) return q; }
        ATN_HIP(hipMemcpyAsync(out, reinterpret_cast<char*>(nodes.p) + list_base[list], bytes, hipMemcpyDeviceToHost, stream));
        ATN_HIP(hipStreamSynchronize(stream));
        return ATN_OK;
    }

    // ≙ idaten::Renderer::updateCamera, renderer.cpp:202-205
    int updateCamera(const atn_camera_param* c)
    {
        if (!c) return fail(ATN_ERR_INVALID_ARG, "null camera");
        camera = *c;
        has_camera = true;
        return ATN_OK;
    }

    int setRandom(const uint32_t* v, uint32_t n)
    {
        if (!v || n == 0) return fail(ATN_ERR_INVALID_ARG, "empty seed array");
        ATN_HIP(hipSetDevice(device));
        { int q = quiesce(); if (q) return q; }
        ATN_HIP(seeds.resize(n));
        ATN_HIP(hipMemcpyAsync(seeds.p, v, (size_t)n * 4, hipMemcpyHostToDevice, stream));
        ATN_HIP(hipStreamSynchronize(stream));
        n_seeds = n;
        return ATN_OK;
    }

    // ≙ aten::getRandom(), src/libaten/sampler/sampler.cpp:20-23: the table as the kernels read it
    int getRandom(uint32_t* out, uint32_t n)
    {
        if (!out || n == 0 || n > n_seeds) return fail(ATN_ERR_INVALID_ARG, "atn_get_random: null output or more entries than the sampler holds");
        ATN_HIP(hipSetDevice(device));
        { int q = quiesce(); if (q) return q; }
        ATN_HIP(hipMemcpyAsync(out, seeds.p, (size_t)n * 4, hipMemcpyDeviceToHost, stream));
        ATN_HIP(hipStreamSynchronize(stream));
        return ATN_OK;
    }

    // ≙ aten::initSampler, src/libaten/sampler/sampler.cpp:8-18
    int initSampler(int32_t w, int32_t h, int32_t seed)
    {
        if (w <= 0 || h <= 0) return fail(ATN_ERR_INVALID_ARG, "bad sampler size");
        std::vector<uint32_t> v((size_t)w * h);
        std::mt19937 src(seed);
        for (auto& x : v) x = (uint32_t)src();
        return setRandom(v.data(), (uint32_t)v.size());
    }

    int ensure_frame(int32_t w, int32_t h, int32_t max_depth)
    {
        const int32_t tx = (w + 7) / 8, ty = (h + 7) / 8;
        const uint32_t n_tiles = (uint32_t)tx * ty;
        const uint32_t tiles_per_rank = (n_tiles + world - 1) / world;
        const uint32_t slots = tiles_per_rank * 64;
        if (slots > kShadowSlotMask) return fail(ATN_ERR_UNSUPPORTED, "more than 2^26 path slots per GPU (shard the screen)");
        if (slots != n_slots) {
            ATN_HIP(ray_o.resize(slots)); ATN_HIP(ray_d.resize(slots)); ATN_HIP(thr.resize(slots));
            ATN_HIP(contrib.resize(slots)); ATN_HIP(isect.resize(slots));
            ATN_HIP(sh_o.resize(slots)); ATN_HIP(sh_d.resize(slots)); ATN_HIP(sh_c.resize(slots));
            ATN_HIP(accum.resize(slots)); ATN_HIP(done.resize(slots));
            ATN_HIP(queue0.resize(slots)); ATN_HIP(queue1.resize(slots)); ATN_HIP(shadow_q.resize(slots));
            ATN_HIP(tile_out.resize(slots));
            n_slots = slots;
        }
        if (w != film_w || h != film_h) {
            if (frames_in_flight > 1) { int qrc = quiesce(); if (qrc) return qrc; }
            ATN_HIP(film.resize((size_t)w * h));
            ATN_HIP(hipMemsetAsync(film.p, 0, (size_t)w * h * sizeof(float4), stream));
            film_w = w; film_h = h;
        }
        if (max_depth + 2 > counters_depth) {
            ATN_HIP(counters.resize((size_t)kMaxBatches * 4 * (max_depth + 2)));
            counters_depth = max_depth + 2;
        }
        if (!stats.p) {
            ATN_HIP(stats.resize(16));
            ATN_HIP(hipMemsetAsync(stats.p, 0, 128, stream));
        }
        if (!nee_stats.p) {
            ATN_HIP(nee_stats.resize(2));
            ATN_HIP(hipMemsetAsync(nee_stats.p, 0, 16, stream));
            ATN_HIP(hipStreamSynchronize(stream));      // (once per context: every bank's stream adds to it)
        }
        return ATN_OK;
    }

    // batch k's queues live in [slot_begin, slot_end) of the queue arrays (a batch never has more live paths than
    // slots) and its counters in the k-th counter block
    PathBuffers buffers(bool count, int batch = 0, uint32_t slot_begin = 0)
    {
        PathBuffers pb{};
        pb.ray_o = ray_o.p; pb.ray_d = ray_d.p; pb.thr = thr.p; pb.contrib = contrib.p; pb.seeds = seeds.p;
        pb.isect = isect.p; pb.sh_o = sh_o.p; pb.sh_d = sh_d.p; pb.sh_c = sh_c.p;
        pb.accum = accum.p; pb.done = done.p; pb.queue[0] = queue0.p + slot_begin; pb.queue[1] = queue1.p + slot_begin;
        pb.shadow_q = shadow_q.p + slot_begin;
        uint32_t* cb = counters.p + (size_t)batch * 4 * counters_depth;
        pb.q_count = cb; pb.sh_count = cb + counters_depth;
        pb.fetch_closest = cb + 2 * counters_depth; pb.fetch_shadow = cb + 3 * counters_depth;
        pb.stats = count ? stats.p : nullptr;
        pb.cost = count ? cost.p : nullptr;
        return pb;
    }

    FrameParams frame_params(const atn_destination& d)
    {
        FrameParams fp{};
        fp.width = d.width; fp.height = d.height; fp.n_slots = (int32_t)n_slots;
        fp.tiles_x = (d.width + 7) / 8; fp.tiles_y = (d.height + 7) / 8; fp.tiles_x_rcp = udiv_rcp((uint32_t)fp.tiles_x);
        fp.rank = rank; fp.world = world;
        fp.max_depth = d.maxDepth;
        fp.rr_depth = d.russianRouletteDepth;
        if (fp.rr_depth > fp.max_depth) fp.rr_depth = fp.max_depth - 1;    // pathtracing.cpp:282-284
        fp.slot_begin = 0; fp.slot_end = (int32_t)n_slots;
        fp.chunk_items = kChunkItems;
        fp.sample = 0; fp.frame = d.frame; fp.n_seeds = n_seeds;
        fp.break_on_terminate = d.break_on_terminate; fp.progressive = d.progressive;
        return fp;
    }

    // How the renderers built on the serial pass open a frame (ReSTIR, NPR, AO, the shadow pre-pass): the frame's parameters with the
    // plan's shade chunks, the bank's buffers uncounted, one serial pass over every slot
    struct SerialFrame { FrameParams fp; PathBuffers pb; PassPlan plan; };
    SerialFrame serial_frame(const atn_destination& d)
    {
        SerialFrame f{ frame_params(d), buffers(false), plan_pass(PassKind::Serial, n_slots) };
        f.fp.chunk_items = f.plan.shade_items;
        return f;
    }

    // Traversal flavour.  Measured on MI355X: the persistent lane-refilling walk wins
    // on sponza_lod (38 K nodes, ~56 node visits per ray: trace 3.25 -> 2.90 ms, shadow 4.40 -> 3.60 ms per
    // 1080p frame) and loses on the Cornell box (71 nodes, ~20 visits per ray: 0.83 -> 1.18 ms).
    // Since the trace launches are fused (r01-g) the refill walk only pays when a launch carries >= ~1.5 M paths as
    // well: on the 2-, 4- and 8-way shards of the 1080p frame the plain walk is 12-16 % faster (3.28 / 2.10 / 1.48 ms
    // against 3.71 / 2.39 / 1.77), so the flavour is picked per frame from tree size AND frame size.
    bool tree_is_deep = false;
    static constexpr size_t kRefillMinNodes = 2048;
    // Re-measured after the burst walk (r02_e, sponza_lod, 3 frames in flight, ms per frame of an N-way shard: refill 4.29 /
    // 2.31 / 1.29 / 0.71 vs plain 5.51 / 2.93 / 1.39 / 0.75 at 2.07 M / 1.04 M / 0.52 M / 0.26 M paths): the r01 crossover of
    // 1.9 M paths is gone, deep trees take the refill walk at every size that fills the machine at all
    // r04, after the plain walk dropped from 84 to 63 VGPRs (8 waves per SIMD; no SLP pairing): it wins again on the 4- and 8-way shards of a
    // 1080p frame (sponza_lod 1.157 -> 1.097 / 0.640 -> 0.608 ms, atrium 1.753 -> 1.700 / 1.112 -> 1.032 with 3 frames in flight) and loses on
    // the 2-way shard of sponza_lod (2.13 vs 2.21) and on full frames (4.04 vs 4.47): profiles/r04_shard_matrix.txt
    // Re-measured after the refill walk's r04 changes (direct start, rays finished with the refill, TLAS step every third iteration): the two
    // walks tie on the 4-way shard (sponza_lod 1.075 / 1.076 ms, atrium 1.667 refill / 1.704 plain), the plain walk keeps the 8-way shard
    // (0.606 vs 0.627, atrium 1.036 vs 1.075): 800 K -> 400 K paths
    static constexpr uint32_t kRefillMinPaths = 400u * 1000u;
    // the walk of a frame's passes (frame) or of the traversal probe (the tree alone); ATEN_AMD_TRACE forces one for every launch
    bool refill_walk(bool frame) const
    {
        if (env_flavour >= 0) return env_flavour == 1;
        return tree_is_deep && (!frame || n_slots >= kRefillMinPaths);
    }

    // bytes of the LDS copy a small scene is walked from (node image + matrix rows), 0 = the scene is walked from global memory
    uint32_t lds_scene_bytes() const
    {
        const uint64_t b = (uint64_t)scene.node_bytes + (uint64_t)scene.mtx_quads * 16u;
        return (env_lds_nodes && b <= kLdsNodesMaxBytes) ? (uint32_t)b : 0u;
    }

    uint32_t trace_grid(uint32_t n_jobs, bool refill) const
    {
        if (refill) {
            // persistent waves pulling kFetchChunk-job chunks: about as many waves as fit on the chip
            const uint32_t waves_per_block = (uint32_t)kTraceBlock / 64u;
            uint32_t blocks = ((n_jobs + atn::kFetchChunk - 1u) / atn::kFetchChunk + waves_per_block - 1u) / waves_per_block;
            if (blocks < 1u) blocks = 1u;
            // One frame at a time: 8 waves per SIMD's worth (6 are resident at 78 VGPRs; the rest start as those retire: best
            // isolated launch, 3.28 ms of trace per sponza_lod frame).  With frames in flight the other frames' kernels want
            // room beside this launch: 4.5 waves per SIMD's worth is slower alone (3.35 ms) and faster in the pipeline (r04 sweep,
            // profiles/r04_sweep_trace_grid.txt: sponza_lod 4.13 -> 4.04 ms per frame, atrium 5.84 -> 5.71 with 4 frames in flight;
            // 768 .. 1280 blocks within 1 %).
            const uint32_t cap = (frames_in_flight > 1 ? 256u * 18u : 256u * 32u) / waves_per_block;
            return blocks < cap ? blocks : cap;
        }
        return grid_for(n_jobs);
    }

    // What a pass over n paths launches (device/launch.hpp: PassPlan).  The frame's walk, the LDS copy and the shade flavour are
    // properties of the context; the grids and chunk sizes follow n.
    PassPlan plan_pass(PassKind kind, uint32_t n) const
    {
        PassPlan p{};
        p.kind = kind;
        p.refill = refill_walk(true);
        p.lds_bytes = lds_scene_bytes();
        p.sph = n_sphere_leaves > 0;
        // threads per block of the plain walk's fused launches: one wave per block retires on its own (1-2 % over 256); a node image
        // of a few KB is walked from an LDS copy (trace_simple<., ., true>), above 8 KB per copy the blocks get four waves to share it
        p.block = p.lds_bytes > 8192u ? 256u : 64u;
        p.trace_grid = trace_grid(n, p.refill);
        p.fused_grid = trace_grid(2u * n, p.refill);
        // k_shade works on chunks of `items` x 256 queue entries per block (one queue atomic per chunk): 4 on full
        // frames; below ~0.4 M paths a launch has too few such blocks to fill 256 CUs (measured on the 8-way
        // shard: 2 -> 1.38 ms, 4 -> 1.46 ms, 1 -> 1.41 ms per frame)
        p.shade_items = n >= 400u * 1000u ? kChunkItems : 2;
        p.shade_grid = grid_for((n + (uint32_t)p.shade_items - 1u) / (uint32_t)p.shade_items);
        // 5 waves per SIMD (96 registers, a few spilled) pays where shade shares the SIMDs with another frame's trace waves AND the launch is
        // large enough not to be latency-bound itself: the Disney / analytic sets on every shard size measured, the core set on full frames
        // only (profiles/r04_variants_shade_waves.txt, r04_shard_matrix.txt).  The SVGF flavour -- AOV writes, 25 registers spilled at 96 --
        // stays at 4 (C5 4.66 vs 4.68 ms per frame), and so does the regenerated shade kernel, which needs all 128 registers of the 4-wave
        // budget (held to 96 for 5 waves it spills 21-44 of them).
        const bool big = n >= 1500u * 1000u;
        p.shade_waves = env_shade_waves ? env_shade_waves
                      : (kind == PassKind::Serial && frames_in_flight > 1 && (scene.material_set != kMsCore || big) ? 5 : 4);
        return p;
    }

    // the unfused trace launches (ATEN_AMD_FUSE=0, and counted frames: the fused kernel does not count); the persistent kernels run
    // kTraceBlock threads per block
    template <bool SHADOW>
    void launch_trace(const PassPlan& p, const PathBuffers& pb, bool count, int32_t b, hipStream_t st)
    {
        const dim3 g(p.trace_grid), t(p.refill ? (uint32_t)kTraceBlock : 256u);
        if (p.sph) { sph_launch_trace(SHADOW, count, p.refill, g.x, t.x, st, pb, scene, b); return; }
        with_flags([&](auto c, auto refill) {
            if constexpr (SHADOW) hipLaunchKernelGGL((k_trace_shadow<decltype(c)::value, decltype(refill)::value>), g, t, 0, st, pb, scene, b);
            else hipLaunchKernelGGL((k_trace_closest<decltype(c)::value, decltype(refill)::value>), g, t, 0, st, pb, scene, b);
        }, count, p.refill);
    }

    // Does this frame of render() run the roulette look-ahead (kernels.hpp, F_DOOMED)?  The scene has to qualify (DevScene::rr_lookahead);
    // counted frames stay the reference's own accounting unless mode 2 asks for the look-ahead's; the relaxed-math shade kernel (not
    // the parity path) has no look-ahead flavour.
    bool rr_lookahead_frame(bool count) const
    {
        return rr_lookahead >= (count ? 2 : 1) && scene.rr_lookahead != 0 && !shade_math_relaxed && scene.material_set <= kMsAnalytic;
    }
    // Does this frame of render() defer its NEE evaluation (kernels.hpp, PathBuffers::nee_reached)?  The scene has to qualify, and under
    // the default policy (mode 2) every light has to be infinite (DevScene::nee_deferral); counted frames stay eager -- their shadow-ray
    // counter is the reference's, which casts no ray for a sample whose BSDF pdf is 0 -- and the relaxed-math kernel has no such flavour.
    bool nee_deferral_frame(bool count) const
    {
        const int32_t need = nee_deferral == 1 ? 1 : 3;
        return nee_deferral != 0 && !count && (scene.nee_deferral & need) == need && !shade_math_relaxed && scene.material_set <= kMsAnalytic;
    }
    // k_nee_eval for bounce b of a deferred frame: behind the trace launch that carried b's shadow rays
    void launch_nee_eval(uint32_t grid, hipStream_t st, const PathBuffers& pb, const FrameParams& fp, int32_t b)
    {
        with_shade_flavour(scene.material_set, 4, [&](auto k) {
            using K = decltype(k);
            if constexpr (K::waves != 0) hipLaunchKernelGGL((k_nee_eval<K::ms>), dim3(grid), dim3(256), 0, st, pb, scene, fp, b, nee_stats.p);
        });
    }

    template <bool SVGF>
    void launch_shade(const PassPlan& p, hipStream_t st, const PathBuffers& pb, const FrameParams& fp, int32_t b, const SvgfShade& sv)
    {
        if (!SVGF && shade_math_relaxed) {      // atn_set_shade_math(1): the same kernel under --use_fast_math rules (shade_relaxed.hip); not the parity path
            relaxed_launch_shade(scene.material_set, p.shade_waves, p.shade_grid, st, pb, scene, fp, camera, b);
            return;
        }
        // the look-ahead's flavour from the first launch that can mark a path (bounce + 1 > rr_depth) on; the launches before it are the
        // kernel as it is without -- and so is every launch of a material set that has no such flavour (none of those qualifies:
        // rr_lookahead_frame; unmarked, no path is ever doomed)
        const bool la = !SVGF && pb.doomed_bit != 0u && b >= fp.rr_depth;
        if (!SVGF && p.sph) { (void)sph_launch_shade(scene.material_set, p.shade_waves, la, p.shade_grid, st, pb, scene, fp, camera, b); return; }     // (sph_frame_check refused what has no such kernel)
        // the deferred-NEE flavour for every launch of a deferred frame (nee_deferral_frame: run_paths hands such a frame the flag plane)
        const bool dn = !SVGF && pb.nee_reached != nullptr;
        with_shade_flavour(scene.material_set, p.shade_waves, [&](auto k) {
            using K = decltype(k);
            if constexpr (!SVGF && K::waves != 0) {
                if (la || dn) {
                    with_flags([&](auto f_la, auto f_dn) {
                        hipLaunchKernelGGL((k_shade_wn<false, K::ms, K::waves, decltype(f_la)::value, decltype(f_dn)::value>), dim3(p.shade_grid), dim3(256), 0, st,
                                           pb, scene, fp, camera, b, sv);
                    }, la, dn);
                    return;
                }
            }
            if constexpr (K::waves == 0) hipLaunchKernelGGL((k_shade<SVGF, K::ms>), dim3(p.shade_grid), dim3(256), 0, st, pb, scene, fp, camera, b, sv);
            else hipLaunchKernelGGL((k_shade_wn<SVGF, K::ms, K::waves>), dim3(p.shade_grid), dim3(256), 0, st, pb, scene, fp, camera, b, sv);
        });
    }

    void prof_begin(bool on, int kind, hipStream_t st = nullptr)
    {
        if (!st) st = stream;
        prof_stream = st;
        if (!on) return;
        if (spans.size() >= kMaxSpans) {    // nobody collected for thousands of launches: resolve them now (bounded pool)
            (void)hipStreamSynchronize(stream);
            for (int k = 0; k < kMaxBatches; k++) (void)hipStreamSynchronize(bstream[k]);
            prof_collect();
        }
        if (ev_used + 2 > ev_pool.size()) {
            for (int i = 0; i < 64; i++) { ev_pool.emplace_back(); (void)hipEventCreate(&ev_pool.back().h); }
        }
        spans.push_back(Span{ kind, ev_used, ev_used + 1 });
        (void)hipEventRecord(ev_pool[ev_used], st);
    }
    void prof_end(bool on)
    {
        if (!on) return;
        (void)hipEventRecord(ev_pool[ev_used + 1], prof_stream);
        ev_used += 2;
    }
    void prof_collect()
    {
        for (const Span& s : spans) {
            float ms = 0;
            if (hipEventElapsedTime(&ms, ev_pool[s.e0], ev_pool[s.e1]) == hipSuccess) { k_ms[s.kind] += ms; k_launches[s.kind]++; }
        }
        spans.clear();
        ev_used = 0;
    }

    // The sample loop of OnRender for every batch of the frame, each on its own stream, forked from and joined
    // back into `stream`.  SVGF = the SVGFRenderer flavour (AOV-writing shade, its own sample epilogue).
    template <bool SVGF>
    int run_paths(const atn_destination* d, FrameParams fp, bool count, bool prof, const SvgfShade& sv, const SvgfFrame& sf)
    {
        // Measured policy (sponza_lod / Cornell 1080p and its 2-, 4-, 8-way shards): overlap pays
        // while launches are latency-bound (<= ~1 M paths in flight); on a full 1080p frame the concurrent shade kernel
        // streams path state through the L2 that the walk wants for its nodes and the deep-tree walk loses more than
        // the overlap wins (6.13 vs 6.59 ms), the shallow-tree walk still gains with two batches.
        int nb;
        if (batches_forced) {
            nb = n_batches;
            const uint32_t min_batch = 200u * 1000u;
            while (nb > 1 && n_slots / (uint32_t)nb < min_batch) nb--;
        }
        else {
            // the refill walk wants the machine to itself; the plain walk gains from a second batch down to ~0.8 M paths
            // (with frames in flight the next frame fills the gaps a second batch was for: measured r02_e on Cornell, 3 in
            // flight, 1.04 M paths: 1 batch 0.82 ms, 2 batches 0.96; 2.07 M paths: 1.66 vs 1.63)
            // (r03, node image in LDS, 3 in flight, Cornell 2.07 M paths: 1 batch 1.52 ms, 2 batches 1.58 -- one batch whenever frames overlap)
            nb = refill_walk(true) ? 1 : (lds_scene_bytes() && frames_in_flight > 1) ? 1 : (n_slots >= (frames_in_flight > 1 ? 1500u : 800u) * 1000u ? 2 : 1);
            if (nb > n_batches) nb = n_batches;
        }
        // the streams a frame's batches run on must not share a hardware queue (see streams_run_side_by_side)
        if (nb > batch_streams_checked && nb > 1 && env_probe_streams) { int rc = separate_batch_streams(nb); if (rc) return rc; }
        uint32_t per = (n_slots + (uint32_t)nb - 1u) / (uint32_t)nb;
        per = (per + kChunk - 1u) / kChunk * kChunk;        // whole 1024-slot chunks (16 screen tiles)
        // A deferred-NEE frame's extra state -- the second plane of hit records, sh_w, the flag words: 36 B per slot -- is allocated
        // when a bank first runs such a frame (DevBuf::resize frees behind the device's work and never shrinks); a context that
        // stays in mode 0, and every other renderer, never pays for it.
        const bool deferred = !SVGF && nee_deferral_frame(count);
        if (deferred) {
            ATN_HIP(isect.resize((size_t)2 * n_slots)); ATN_HIP(sh_w.resize(n_slots)); ATN_HIP(nee_reached.resize(n_slots));
        }
        ATN_HIP(hipMemsetAsync(counters.p, 0, (size_t)nb * 4 * counters_depth * 4, stream));
        ATN_HIP(hipEventRecord(ev_fork, stream));
        for (int k = 0; k < nb; k++) {
            const uint32_t begin = (uint32_t)k * per;
            const uint32_t end = begin + per < n_slots ? begin + per : n_slots;
            if (begin >= end) continue;
            hipStream_t st = nb > 1 ? bstream[k] : stream;
            if (nb > 1) ATN_HIP(hipStreamWaitEvent(st, ev_fork, 0));
            PathBuffers pb = buffers(count, k, begin);
            pb.doomed_bit = (!SVGF && rr_lookahead_frame(count)) ? F_DOOMED : 0u;
            pb.doomed_stop = rr_lookahead_twin ? kInf : 1.0e30F;        // (kInf is the largest finite float: any smaller bound beyond every scene's distances stops the walk and is not the twins' key)
            if (deferred) { pb.isect_odd = n_slots; pb.nee_reached = nee_reached.p; pb.sh_w = sh_w.p; }
            fp.slot_begin = (int32_t)begin; fp.slot_end = (int32_t)end;
            const uint32_t n = end - begin;
            const PassPlan plan = plan_pass(SVGF ? PassKind::Svgf : PassKind::Serial, n);
            fp.chunk_items = plan.shade_items;
            const uint32_t g_slots = grid_for(n), g_all = (n + 255u) / 256u;
            // k_nee_eval: a block per four 1024-entry chunks of a full shadow queue (never 0) -- enough flagged entries per block for
            // full replay waves where a few per cent of the rays reach the light, enough blocks to cover the chip on a 1080p frame
            const uint32_t g_nee = grid_for((n + 4u * kChunk - 1u) / (4u * kChunk) * 256u);
            for (int32_t s = 0; s < d->sample; s++) {
                fp.sample = s;
                if (s > 0) ATN_HIP(hipMemsetAsync(pb.q_count, 0, (size_t)4 * counters_depth * 4, st));
                prof_begin(prof, ATN_K_GEN, st);
                hipLaunchKernelGGL(k_gen_path, dim3(g_slots), dim3(256), 0, st, pb, fp, camera, (const uint32_t*)seeds.p);
                prof_end(prof);
                if (count || !fuse_traces) {
                    for (int32_t b = 0; b < d->maxDepth; b++) {
                        prof_begin(prof, ATN_K_TRACE_CLOSEST, st);
                        launch_trace<false>(plan, pb, count, b, st);
                        prof_end(prof);
                        if (SVGF && b == 0 && gm_capture) motion_launch_capture(g_all, st, pb, fp, gm_capture);
                        prof_begin(prof, ATN_K_SHADE, st);
                        launch_shade<SVGF>(plan, st, pb, fp, b, sv);
                        prof_end(prof);
                        prof_begin(prof, ATN_K_TRACE_SHADOW, st);
                        launch_trace<true>(plan, pb, count, b, st);
                        prof_end(prof);
                        if (deferred) {
                            prof_begin(prof, ATN_K_TRACE_SHADOW, st);       // (with the shadow launch whose rays it evaluates, as in the fused loop)
                            launch_nee_eval(g_nee, st, pb, fp, b);
                            prof_end(prof);
                        }
                    }
                }
                else {
                    // depth + 1 trace launches: [closest 0], [shadow b + closest b+1] ..., [shadow depth-1]
                    for (int32_t b = 0; b <= d->maxDepth; b++) {
                        const TraceLaunch tl = trace_launch(plan, b);
                        prof_begin(prof, tl.prof_kind, st);
                        launch_trace_fused<false>(tl, st, pb, scene, b - 1, b < d->maxDepth ? b : -1, b);
                        prof_end(prof);
                        if (SVGF && b == 0 && gm_capture) motion_launch_capture(g_all, st, pb, fp, gm_capture);
                        // deferred NEE: the launch above carried the shadow rays of bounce b - 1; their evaluation goes in front of
                        // whatever vertex b adds to `contrib` (and, behind the last launch, in front of the sample's epilogue)
                        if (deferred && b > 0) {
                            prof_begin(prof, ATN_K_TRACE_SHADOW, st);       // (HitShadowRay's addition: timed apart from the shade launches)
                            launch_nee_eval(g_nee, st, pb, fp, b - 1);
                            prof_end(prof);
                        }
                        if (b < d->maxDepth) {
                            prof_begin(prof, ATN_K_SHADE, st);
                            launch_shade<SVGF>(plan, st, pb, fp, b, sv);
                            prof_end(prof);
                        }
                    }
                }
                if (SVGF || d->sample > 1) {     // with one sample per pixel k_gather<true> does the epilogue itself
                    prof_begin(prof, ATN_K_ACCUM, st);
                    if (SVGF) hipLaunchKernelGGL(k_svgf_sample_end, dim3(g_all), dim3(256), 0, st, pb, fp, sf);
                    else hipLaunchKernelGGL(k_accumulate_sample, dim3(g_all), dim3(256), 0, st, pb, fp);
                    prof_end(prof);
                }
            }
            if (nb > 1) {
                ATN_HIP(hipEventRecord(ev_join[k], st));
                ATN_HIP(hipStreamWaitEvent(stream, ev_join[k], 0));
            }
        }
        return ATN_OK;
    }

    // ---- what every frame does around its passes (render, render_regen, svgf_render) ----
    int check_ready(const atn_destination* d)
    {
        if (!d) return fail(ATN_ERR_INVALID_ARG, "null destination");
        if (!has_scene) return fail(ATN_ERR_NO_SCENE, "atn_upload_scene has not been called");
        if (!has_camera) return fail(ATN_ERR_INVALID_ARG, "atn_update_camera has not been called");
        if (n_seeds == 0) return fail(ATN_ERR_INVALID_ARG, "atn_init_sampler / atn_set_random has not been called");
        if (d->width <= 0 || d->height <= 0 || d->maxDepth <= 0 || d->sample <= 0) return fail(ATN_ERR_INVALID_ARG, "bad destination");
        return ATN_OK;
    }
    // rotate (the bank that has been idle longest becomes the current one), go behind the latest scene update, size the buffers
    int begin_frame(const atn_destination& d, bool rotate)
    {
        if (rotate) swap_bank(spare[frame_seq % (uint64_t)(frames_in_flight - 1)]);
        frame_seq++;
        const int rc = wait_scene_epoch();
        return rc ? rc : ensure_frame(d.width, d.height, d.maxDepth);
    }
    // the film is a running mean: its writers go in frame order, each behind the last one (ev_film)
    int wait_film()
    {
        if (film_pending) ATN_HIP(hipStreamWaitEvent(stream, ev_film, 0));
        return taa_before_write(stream);        // (a display tail that still reads the film: atn_taa_resolve, source 1)
    }
    int record_film_writer()
    {
        if (frames_in_flight <= 1) return ATN_OK;
        if (!ev_film) ATN_HIP(hipEventCreateWithFlags(&ev_film.h, hipEventDisableTiming));
        ATN_HIP(hipEventRecord(ev_film, stream));
        film_pending = true;
        return ATN_OK;
    }
    // a frame's accumulated samples into the film, behind the film's last writer (with one sample per pixel k_gather<true> does the
    // sample's epilogue itself)
    int gather_film(const atn_destination& d, const PathBuffers& pb, const FrameParams& fp)
    {
        const int rc = wait_film();
        if (rc) return rc;
        const uint32_t g_all = (n_slots + 255u) / 256u;
        prof_begin(d.profile != 0, ATN_K_GATHER);
        if (d.sample == 1) hipLaunchKernelGGL((k_gather<true>), dim3(g_all), dim3(256), 0, stream, pb, fp, film.p, tile_out.p);
        else hipLaunchKernelGGL((k_gather<false>), dim3(g_all), dim3(256), 0, stream, pb, fp, film.p, tile_out.p);
        prof_end(d.profile != 0);
        ATN_HIP(hipGetLastError());
        return ATN_OK;
    }
    int end_film_frame()
    {
        const int rc = frames_in_flight > 1 ? record_scene_read() : ATN_OK;
        return rc ? rc : record_film_writer();
    }
    // ... and the film in host memory, if the caller asked for it
    int end_film_frame(const atn_destination& d, atn_vec4* out_host)
    {
        const int rc = end_film_frame();
        if (rc || !out_host) return rc;
        ATN_HIP(hipMemcpyAsync(out_host, film.p, (size_t)d.width * d.height * sizeof(float4), hipMemcpyDeviceToHost, stream));
        ATN_HIP(hipStreamSynchronize(stream));
        return ATN_OK;
    }

    // ≙ idaten::PathTracing::render + OnRender (src/libidaten/kernel/pathtracing.cpp:49-153), loop
    // structure of aten::PathTracing::OnRender/radiance (src/libaten/renderer/pathtracing/pathtracing.cpp:22-89,269-366)
    int render(const atn_destination* d, atn_vec4* out_host)
    {
        int rc = check_ready(d);
        if (rc) return rc;
        rc = ns_check(d);
        if (rc) return rc;
        rc = sph_frame_check(*d);
        if (rc) return rc;
        ATN_HIP(hipSetDevice(device));
        if (d->sample > 1 && regen_applies(*d, 1)) return render_regen(d, 1, out_host);
        const bool count = d->count_stats != 0, prof = d->profile != 0;
        if (frames_in_flight > 1 && count) { rc = quiesce(); if (rc) return rc; }      // the counters are one set, read back synchronously
        rc = begin_frame(*d, frames_in_flight > 1 && !count);
        if (rc) return rc;
        FrameParams fp = frame_params(*d);
        if (count) {
            ATN_HIP(hipMemsetAsync(stats.p, 0, 128, stream));
            ATN_HIP(cost.resize((size_t)2 * n_slots));
            ATN_HIP(cost_film.resize((size_t)2 * d->width * d->height));
            ATN_HIP(hipMemsetAsync(cost.p, 0, (size_t)2 * n_slots * sizeof(uint32_t), stream));
            ATN_HIP(hipMemsetAsync(cost_film.p, 0, (size_t)2 * d->width * d->height * sizeof(uint32_t), stream));
            cost_w = d->width; cost_h = d->height;
        }
        PathBuffers pb = buffers(count);

        const uint32_t g_all = (n_slots + 255u) / 256u;
        // atn_npr_shadow_set_mode(1): this frame's Toon shading reads the plane the pre-pass makes now
        if (ns_frame()) { rc = ns_prepass(d); if (rc) return rc; }
        rc = run_paths<false>(d, fp, count, prof, SvgfShade{}, SvgfFrame{});
        { const int e = ns_end_frame(); if (!rc) rc = e; }
        if (rc) return rc;
        fp.slot_begin = 0; fp.slot_end = (int32_t)n_slots;
        rc = gather_film(*d, pb, fp);
        if (rc) return rc;
        rc = end_film_frame();
        if (rc) return rc;

        if (count) {
            hipLaunchKernelGGL(k_cost_to_pixels, dim3(g_all), dim3(256), 0, stream, fp, (const uint32_t*)cost.p, cost_film.p);
            ATN_HIP(hipMemcpyAsync(host_stats, stats.p, 128, hipMemcpyDeviceToHost, stream));
        }
        if (out_host) {
            ATN_HIP(hipMemcpyAsync(out_host, film.p, (size_t)d->width * d->height * sizeof(float4), hipMemcpyDeviceToHost, stream));
        }
        if (out_host || count) ATN_HIP(hipStreamSynchronize(stream));
        if (count) {
            // the closest-hit kernels count every ray of their queue: the doomed ones (mode 2 only, else zero) are reported on their own
            host_stats[0] -= host_stats[8]; host_stats[3] -= host_stats[10]; host_stats[4] -= host_stats[11];
        }
        return ATN_OK;      // profiling spans are resolved lazily in kernel_times() (no sync in the frame loop)
    }


    // ------------------------------------------------------------------------------------------------
    // Path regeneration (BASELINE.json north_star "path compaction/regeneration"; atn_set_regeneration, atn_render_burst).
    //
    // The serial loop above -- the reference's, src/libidaten/kernel/pathtracing.cpp:105-138 -- is `for sample { generate; for bounce
    // { trace; shade } ; accumulate } gather`: every launch of a sample works on what is left of the population after the bounces
    // before it, a pixel whose path ended early idles until the longest path of the sample is over, and the next sample (or the next
    // progressive frame) starts from an empty machine.  Here one POOL of slots -- a slot is a pixel -- runs a whole burst of
    // `n_frames` progressive frames x `spp` samples: `begin; for stage { trace; shade } ; end`.  A path that ends in shade(stage)
    // has its sample epilogue run there (accumulate; after the frame's last sample Film::put), and the pixel's next primary ray is
    // written into the same slot and queued for trace(stage + 1); bounce, sample and frame are per-path state (kernels.hpp).  Per
    // pixel the samples and frames follow each other in the serial order with the serial operations, so films are BYTE-equal to
    // the serial loop's (tests/test_gpu_regen.py); what changes is only which launch a piece of work rides in.
    //
    // A path that runs out of depth with a shadow ray to trace hands its contribution over (`pend`) and the next sample starts at
    // once; the shadow ray adds its light to `pend` in the next stage's trace launch and the epilogue runs at the start of that
    // stage's shade (F_PENDING) -- before anything of the new sample can reach accum or the film.
    //
    // The film itself is written once per burst, by k_regen_end, from the burst's staging planes (one pixel value per frame): only that
    // launch is ordered behind the previous burst's (ev_film), so bursts on different banks (atn_set_frames_in_flight) overlap like
    // serial frames in flight do.  A burst is cut into pieces of at most kRegenStagingBytes of staging planes.
    //
    // Stages are launched up to the bound n_frames * spp * maxDepth (a pixel's worst case); the kernels read their counts from
    // device memory, and a stage whose queue is empty costs a kernel start.
    // ------------------------------------------------------------------------------------------------
    bool shade_math_relaxed = false;    // atn_set_shade_math
    // atn_render on a scene with sphere leaves: the serial loop with the parity shade math, eager NEE, no pre-pass, no toon surfaces,
    // no material a shadow ray looks through (the sphere-aware kernels of spheres.hip are those)
    int sph_frame_check(const atn_destination& d)
    {
        if (!n_sphere_leaves) return ATN_OK;
        const bool count = d.count_stats != 0;
        if (d.sample > 1 && regen_applies(d, 1)) return sph_refuse("path regeneration does not trace sphere leaves: atn_set_regeneration(0)");
        if (shade_math_relaxed) return sph_refuse("there is no relaxed-math shade kernel for sphere hits: atn_set_shade_math(0)");
        if (nee_deferral_frame(count)) return sph_refuse("deferred NEE does not replay sphere hits: atn_set_nee_deferral(0)");
        if (gm_on) return sph_refuse("geometry motion does not follow sphere leaves: atn_set_geometry_motion(0)");
        if (ns_mode != 0) return sph_refuse("the NPR shadow / hatching pre-pass does not trace sphere leaves: atn_npr_shadow_set_mode(0)");
        if (scene.material_set >= kMsToon) return sph_refuse("toon / stylised materials walk a visibility ray of their own that does not test sphere leaves");
        if (scene.any_alpha) return sph_refuse("shadow rays do not look through alpha / stencil materials in a scene with sphere leaves");
        return ATN_OK;
    }
    int regen_mode = 0;         // atn_set_regeneration: 0 = serial sample loop, 1 = regenerated pool wherever it applies
    uint64_t rg_host_totals[4] = {};
    static constexpr int32_t kRegenMaxStages = 1 << 16;
    static constexpr int32_t kRegenMaxDepth = 128;      // 4096 CMJ dimensions / 32 per bounce (kRegenDimMask)
    static constexpr size_t kRegenStagingBytes = (size_t)1 << 30;

    bool regen_applies(const atn_destination& d, int32_t n_frames) const
    {
        if (regen_mode == 0 || d.count_stats) return false;        // (counted frames use the serial loop's counting kernels)
        if (d.maxDepth > kRegenMaxDepth || (uint32_t)d.sample >= kRegenMaxSpp) return false;
        if ((uint64_t)n_frames * (uint64_t)d.width * (uint64_t)d.height >= kRegenMaxItems) return false;     // (items are 28-bit)
        if (n_frames > 1 && !d.progressive) return false;           // (a burst of overwriting frames is its last frame)
        return ((int64_t)n_frames + 1) * d.sample * d.maxDepth <= kRegenMaxStages;
    }

    // ≙ n_frames x (idaten::PathTracing::render, pathtracing.cpp:49-153) with frame = d->frame, d->frame + 1, ...
    int render_burst(const atn_destination* d, int32_t n_frames, atn_vec4* out_host)
    {
        if (!d) return fail(ATN_ERR_INVALID_ARG, "null destination");
        if (n_frames <= 0) return fail(ATN_ERR_INVALID_ARG, "bad burst length");
        { const int sr = sph_refuse("atn_render_burst does not trace sphere leaves: render the frames with atn_render"); if (sr) return sr; }
        if (ns_mode == 1) return fail(ATN_ERR_UNSUPPORTED, "NPR shadow pre-pass: bursts are not supported: render the frames with atn_render, or atn_npr_shadow_set_mode(0)");
        if (regen_applies(*d, n_frames)) {
            { const int rc = check_ready(d); if (rc) return rc; }
            ATN_HIP(hipSetDevice(device));
            // pieces of at most kRegenStagingBytes of staging planes (1080p: 32 frames; a 4K frame is 133 MB)
            const uint64_t tiles = (uint64_t)((d->width + 7) / 8) * ((d->height + 7) / 8);
            const uint64_t plane = ((tiles + world - 1) / world) * 64u * sizeof(float4);
            int32_t piece = (int32_t)(kRegenStagingBytes / (plane ? plane : 1u));
            if (piece < 1) piece = 1;
            atn_destination part = *d;
            for (int32_t k = 0; k < n_frames; k += piece) {
                const int32_t n = n_frames - k < piece ? n_frames - k : piece;
                part.frame = d->frame + (uint32_t)k;
                const int rc = render_regen(&part, n, k + n == n_frames ? out_host : nullptr);
                if (rc) return rc;
            }
            return ATN_OK;
        }
        atn_destination one = *d;
        for (int32_t k = 0; k < n_frames; k++) {
            one.frame = d->frame + (uint32_t)k;
            const int rc = render(&one, k + 1 == n_frames ? out_host : nullptr);
            if (rc) return rc;
        }
        return ATN_OK;
    }

    int render_regen(const atn_destination* d, int32_t n_frames, atn_vec4* out_host)
    {
        const bool prof = d->profile != 0;
        int rc = begin_frame(*d, frames_in_flight > 1);
        if (rc) return rc;
        // Stages: while items are left every slot is busy, so the cursor passes the last item after at most (path-stages of all items) /
        // (slots) <= n_frames * spp * maxDepth stages; the items then in flight need at most spp * maxDepth more.
        const int32_t stages = (n_frames + 1) * d->sample * d->maxDepth;
        rc = regen_valid_list(d->width, d->height);
        if (rc) return rc;
        if (pend.n < n_slots) ATN_HIP(pend.resize(n_slots));
        const size_t cstride = (size_t)stages + 3;        // counters of stages -1 .. stages + 1
        if (rg_counters.n < 3 * cstride + 1) ATN_HIP(rg_counters.resize(3 * cstride + 1));
        if (rg_frames.n < (size_t)n_frames * n_slots) ATN_HIP(rg_frames.resize((size_t)n_frames * n_slots));
        rg_stages = stages;
        FrameParams fp = frame_params(*d);
        fp.burst_frames = n_frames; fp.spp = d->sample;
        fp.n_valid = rg_n_valid; fp.n_valid_rcp = udiv_rcp(rg_n_valid); fp.n_items = rg_n_valid * (uint32_t)n_frames;
        PathBuffers pb = buffers(false);
        pb.pend = pend.p;
        pb.valid_list = rg_valid.p; pb.next_item = rg_counters.p + 3 * cstride;
        pb.q_count = rg_counters.p + 1; pb.sh_count = rg_counters.p + cstride + 1; pb.fetch_closest = rg_counters.p + 2 * cstride + 1;
        pb.fetch_shadow = nullptr;
        const RegenOut ro{ rg_frames.p, film.p, tile_out.p };

        const uint32_t n = rg_n_valid;      // the pool: one slot per pixel of the shard (n_frames >= 1: never more slots than items)
        const PassPlan plan = plan_pass(PassKind::Regen, n);
        fp.chunk_items = plan.shade_items;
        const uint32_t g_all = (n_slots + 255u) / 256u;
        // the regions a shade launch writes for the compaction in front of the next stage (kernels.hpp, k_regen_compact)
        const uint32_t chunk_size = 256u * (uint32_t)plan.shade_items, n_chunks = (n + chunk_size - 1u) / chunk_size, n_groups = (n_chunks + kRegenGroup - 1u) / kRegenGroup;
        const size_t region_words = (size_t)n_chunks * chunk_size;
        const size_t rg_words = 2 * region_words + 2 * (size_t)n_chunks + 4 * (size_t)n_groups;
        if (rg_regions.n < rg_words) ATN_HIP(rg_regions.resize(rg_words));
        pb.q_regions = rg_regions.p; pb.sh_regions = rg_regions.p + region_words; pb.region_counts = rg_regions.p + 2 * region_words;
        uint32_t* const group_counts[2] = { pb.region_counts + 2 * (size_t)n_chunks, pb.region_counts + 2 * (size_t)n_chunks + 2 * (size_t)n_groups };

        ATN_HIP(hipMemsetAsync(rg_counters.p, 0, (3 * cstride + 1) * sizeof(uint32_t), stream));
        ATN_HIP(hipMemsetAsync(group_counts[0], 0, 4 * (size_t)n_groups * sizeof(uint32_t), stream));
        prof_begin(prof, ATN_K_GEN);
        pb.group_counts = group_counts[0];
        regen_launch_begin(plan.shade_grid, stream, pb, fp, camera);
        regen_launch_compact(n_chunks, stream, pb, 0, chunk_size, group_counts[1], n_groups);
        prof_end(prof);
        for (int32_t i = 0; i <= stages; i++) {
            // trace(i): the shadow rays shade(i - 1) cast + the closest-hit rays of the paths (continued and regenerated) it queued
            const TraceLaunch tl = trace_launch(plan, i);
            prof_begin(prof, tl.prof_kind);
            regen_launch_trace(tl, stream, pb, scene, i - 1, i < stages ? i : -1, i);
            prof_end(prof);
            if (i < stages) {
                prof_begin(prof, ATN_K_SHADE);
                pb.group_counts = group_counts[(i + 1) & 1];
                regen_launch_shade(scene.material_set, plan.shade_waves, plan.shade_grid, stream, pb, scene, fp, camera, i, ro);
                prof_end(prof);
                prof_begin(prof, ATN_K_ACCUM);      // (timed under the serial loop's per-sample epilogue kind)
                regen_launch_compact(n_chunks, stream, pb, i + 1, chunk_size, group_counts[i & 1], n_groups);
                prof_end(prof);
            }
        }
        rc = wait_film();
        if (rc) return rc;
        prof_begin(prof, ATN_K_GATHER);
        regen_launch_flush((n + 255u) / 256u, stream, pb, fp, ro);
        regen_launch_end(g_all, stream, pb, fp, ro);
        prof_end(prof);
        ATN_HIP(hipGetLastError());
        return end_film_frame(*d, out_host);
    }

    // The shard's pixel slots that lie inside the frame, ascending (kernels.hpp: the items of a burst index it).  Built on the host from
    // the tile geometry once per (size, shard) and shared by every bank.
    DevBuf<uint32_t> rg_valid;
    uint32_t rg_n_valid = 0;
    int32_t rg_valid_key[4] = { -1, -1, -1, -1 };
    int regen_valid_list(int32_t w, int32_t h)
    {
        if (rg_valid_key[0] == w && rg_valid_key[1] == h && rg_valid_key[2] == rank && rg_valid_key[3] == world && rg_valid.p) return ATN_OK;
        const int32_t tx = (w + 7) / 8, ty = (h + 7) / 8;
        std::vector<uint32_t> v;
        v.reserve(n_slots);
        for (uint32_t slot = 0; slot < n_slots; slot++) {
            const uint32_t tile = (slot >> 6) * (uint32_t)world + (uint32_t)rank;       // slot_to_pixel, kernels.hpp
            if (tile >= (uint32_t)(tx * ty)) continue;
            const int32_t x = (int32_t)(tile % (uint32_t)tx) * 8 + (int32_t)(slot & 7u), y = (int32_t)(tile / (uint32_t)tx) * 8 + (int32_t)((slot & 63u) >> 3);
            if (x < w && y < h) v.push_back(slot);
        }
        { int q = quiesce(); if (q) return q; }        // (other banks' bursts may be reading the old list)
        ATN_HIP(rg_valid.resize(v.size() ? v.size() : 1));
        ATN_HIP(hipMemcpy(rg_valid.p, v.data(), v.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        rg_n_valid = (uint32_t)v.size();
        rg_valid_key[0] = w; rg_valid_key[1] = h; rg_valid_key[2] = rank; rg_valid_key[3] = world;
        return ATN_OK;
    }

    // per-stage populations of the current bank's last regenerated burst: closest-hit rays and shadow rays of every stage
    int regen_stage_counts(uint32_t* closest, uint32_t* shadow, uint32_t capacity, uint32_t* n_stages)
    {
        ATN_HIP(hipSetDevice(device));
        ATN_HIP(hipStreamSynchronize(stream));
        const uint32_t ns = (uint32_t)rg_stages + 1u;
        if (n_stages) *n_stages = rg_stages > 0 ? ns : 0u;
        if (rg_stages <= 0 || !rg_counters.p) return ATN_OK;
        const size_t cstride = (size_t)rg_stages + 3;
        std::vector<uint32_t> h(2 * cstride);
        ATN_HIP(hipMemcpy(h.data(), rg_counters.p, h.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < ns && i < capacity; i++) {
            if (closest) closest[i] = h[1 + i];
            if (shadow) shadow[i] = h[cstride + 1 + i];
        }
        return ATN_OK;
    }

    // ------------------------------------------------------------------------------------------------
    // SVGF (aten::SVGFRenderer, src/libaten/renderer/svgf/svgf.cpp): frame-persistent state = SVGFParams
    // (svgf_types.h:54-166) + MatricesForRendering (pt_params.h:150-185)
    // ------------------------------------------------------------------------------------------------
    DevBuf<float4> sv_aov[2][4], sv_scratch, sv_atrous[2], sv_tmp, sv_out, sv_stages;
    MotionDepth sv_motion;
    // what the path pass hands to the filters, two slots so that frame f + 1's path pass can run while frame f is filtered:
    // G-buffer staging (normal+depth, albedo+id), primary hit positions, contributions
    DevBuf<float4> sv_gnd[2], sv_gam[2], sv_primary[2], sv_contribs[2];
    int32_t sv_slot = 0, sv_last_slot = 0;      // slot of the next frame / of the last frame, upload or denoise
    DevEvent sv_ev_prepare[2];     // the prepare pass that consumed slot k has finished
    bool sv_prepare_recorded[2] = { false, false };
    float4* sv_cv[2] = { nullptr, nullptr };    // colour+variance of the two AOV sets (the variance pass swaps with sv_spare)
    float4* sv_spare = nullptr;
    int32_t sv_w = 0, sv_h = 0, sv_curr = 0, sv_atrous_iters = 5;
    bool sv_frame_done = false;             // a frame has been rendered / denoised into sv_out at sv_w x sv_h (the display tail's source 0)
    hipStream_t sv_last_fs = nullptr;       // the stream its filter passes ran on
    DevStream sv_stream;        // filter stream of pipelined SVGF frames (frames in flight > 1)
    bool w_or_h_changed(int32_t w, int32_t h) const { return w != sv_w || h != sv_h || w != film_w || h != film_h; }
    DevBuf<float> sv_weight;        // scalar plane of the optional temporal-weight dilation
    int32_t sv_dilate_weight = 0;
    FrameMatrices sv_mtx;

    // ≙ SVGFRenderer::SetMotionDepthBuffer (svgf.cpp:441-450), ReSTIRRenderer::SetMotionDepthBuffer (restir.cpp:472-480) /
    // ReSTIRPathTracing::SetGBuffer's motion-depth texture
    int set_motion_depth(MotionDepth& m, const atn_vec4* md, uint32_t n)
    {
        if (!md || n == 0) return fail(ATN_ERR_INVALID_ARG, "empty motion/depth buffer");
        ATN_HIP(hipSetDevice(device));
        ATN_HIP(m.buf.resize(n));
        ATN_HIP(hipMemcpyAsync(m.buf.p, md, (size_t)n * sizeof(float4), hipMemcpyHostToDevice, stream));
        ATN_HIP(hipStreamSynchronize(stream));
        m.is_set = true;
        m.count = n;
        return ATN_OK;
    }
    // the common opening of the downloads and resets: every frame in flight has finished, and so has `stream`
    int settle()
    {
        ATN_HIP(hipSetDevice(device));
        { int q = quiesce(); if (q) return q; }
        ATN_HIP(hipStreamSynchronize(stream));
        return ATN_OK;
    }
    // ... and their common end: buffer `which` of a renderer's table of stage buffers, behind settle()
    struct StageBuf { const void* p; size_t bytes; };
    template <size_t N>
    int download_stage(const StageBuf (&bufs)[N], int32_t which, void* out, const char* no_such)
    {
        { const int s = settle(); if (s) return s; }
        if (which < 0 || (size_t)which >= N) return fail(ATN_ERR_INVALID_ARG, no_such);
        ATN_HIP(hipMemcpy(out, bufs[which].p, bufs[which].bytes, hipMemcpyDeviceToHost));
        return ATN_OK;
    }

    int fill4(float4* p, size_t n, float4 v)
    {
        hipLaunchKernelGGL(k_svgf_fill, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, stream, p, (uint32_t)n, v);
        return ATN_OK;
    }

    // SVGFParams::InitBuffers: vec4() = (0, 0, 0, 1) for every AOV texel
    int svgf_ensure(int32_t w, int32_t h, bool stages)
    {
        const size_t n = (size_t)w * h;
        if (sv_handover_only) {
            // the hand-over planes as below (same initial values: a pixel the path pass does not write keeps them), and nothing else
            if (w != sv_w || h != sv_h) {
                for (int k = 0; k < 2; k++) {
                    ATN_HIP(sv_primary[k].resize(n)); fill4(sv_primary[k].p, n, make_float4(0, 0, 0, 0));
                    ATN_HIP(sv_contribs[k].resize(n)); ATN_HIP(sv_gnd[k].resize(n)); ATN_HIP(sv_gam[k].resize(n));
                }
                sv_w = w; sv_h = h; sv_curr = 0; sv_slot = 0; sv_last_slot = 0;
                sv_frame_done = false;
            }
            return ATN_OK;
        }
        if (w != sv_w || h != sv_h) {
            const float4 init = make_float4(0.0F, 0.0F, 0.0F, 1.0F);
            for (auto& set : sv_aov) for (auto& b : set) { ATN_HIP(b.resize(n)); fill4(b.p, n, init); }
            ATN_HIP(sv_scratch.resize(n)); fill4(sv_scratch.p, n, init);
            for (auto& b : sv_atrous) { ATN_HIP(b.resize(n)); fill4(b.p, n, init); }
            ATN_HIP(sv_tmp.resize(n)); fill4(sv_tmp.p, n, init);
            for (int k = 0; k < 2; k++) {
                ATN_HIP(sv_primary[k].resize(n)); fill4(sv_primary[k].p, n, make_float4(0, 0, 0, 0));
                ATN_HIP(sv_contribs[k].resize(n)); ATN_HIP(sv_gnd[k].resize(n)); ATN_HIP(sv_gam[k].resize(n));
            }
            ATN_HIP(sv_out.resize(n));
            if (!sv_motion.is_set || sv_motion.count < n) { ATN_HIP(sv_motion.buf.resize(n)); sv_motion.is_set = false; sv_motion.count = 0; }
            sv_cv[0] = sv_aov[0][2].p; sv_cv[1] = sv_aov[1][2].p; sv_spare = sv_scratch.p;
            sv_w = w; sv_h = h; sv_curr = 0; sv_slot = 0; sv_last_slot = 0;
            sv_frame_done = false;
        }
        if (stages) ATN_HIP(sv_stages.resize(3 * n));
        return ATN_OK;
    }

    int svgf_reset()
    {
        sv_w = 0; sv_h = 0; sv_curr = 0;        // buffers are re-initialised by the next svgf_render
        sv_frame_done = false;
        sv_mtx.reset_identity();
        return ATN_OK;
    }

    // uploads address the slot the NEXT frame / denoise call reads, downloads the slot the last one used
    float4* svgf_buffer(int32_t which, bool for_upload = false)
    {
        const int32_t c = sv_curr, p = 1 - sv_curr;
        const int32_t k = for_upload ? sv_slot : sv_last_slot;
        if (for_upload && (which == 10 || which == 14)) sv_last_slot = sv_slot;
        if (which >= 0 && which < 4) return which == 2 ? sv_cv[c] : sv_aov[c][which].p;
        if (which < 8) return which == 6 ? sv_cv[p] : sv_aov[p][which - 4].p;
        switch (which) {
        case 8: return sv_tmp.p; case 9: return sv_motion.buf.p; case 10: return sv_primary[k].p;
        case 11: return sv_atrous[0].p; case 12: return sv_atrous[1].p; case 13: return sv_out.p; case 14: return sv_contribs[k].p;
        case 15: return (!for_upload && gm_sv_ids[k]) ? gm_ids[k].p : nullptr;      // the ids plane of the last mode-2 frame (device/motion.hpp)
        }
        return nullptr;
    }

    // ≙ aten::SVGFRenderer::OnRender (svgf.cpp:452-637): the two halves below, back to back
    int svgf_render(const atn_destination* d, int32_t compute_motion, atn_vec4* out_host, atn_vec4* stages_host, bool path_pass = true)
    {
        { const int sr = sph_refuse("the SVGF renderer does not trace sphere leaves"); if (sr) return sr; }
        int rc = check_ready(d);
        if (rc) return rc;
        // (a shard of a node-wide frame goes through the halves: MultiGpu::svgf_render gathers the hand-over planes in between)
        if (world != 1) return fail(ATN_ERR_UNSUPPORTED, "SVGF needs the whole frame on one GPU (filter footprints cross tiles)");
        rc = svgf_path_half(d, compute_motion, stages_host != nullptr, path_pass);
        return rc ? rc : svgf_filter_half(d, out_host, stages_host);
    }

    // What the path half of an SVGF frame leaves for its filter half: the frame's planes and matrices, the hand-over slot, the stream
    // the filters run on.
    struct SvgfPass {
        SvgfFrame sf{};
        hipStream_t fs = nullptr;
        int32_t slot = 0, cur = 0;
        bool pipelined = false, path_pass = false, prof = false;
    } sv_pass;
    // A shard other than the first of a node-wide frame (MultiGpu::svgf_render) only ever runs the path half: it keeps the hand-over
    // planes and nothing the filters own (AOV sets, moments, a-trous, output, motion, the filter stream).
    bool sv_handover_only = false;
    DevBuf<float4> sv_packed[2];        // ... and, per hand-over slot, its pixels of the four planes packed for the push (k_svgf_pack_tiles)

    // The path half: everything of OnRender up to PrepareForDenoise -- the frame's bank, the planes, the camera matrices, the sample
    // loop into slot sv_slot of the hand-over planes.  Every plane is addressed by pixel (k_shade<SVGF>, k_svgf_sample_end through
    // slot_to_pixel), so on a screen shard (world > 1) it fills exactly the shard's pixels of them.
    int svgf_path_half(const atn_destination* d, int32_t compute_motion, bool want_stages, bool path_pass)
    {
        // (here too: a shard of a node-wide frame enters at this half, not through svgf_render)
        { const int sr = sph_refuse("the SVGF renderer does not trace sphere leaves"); if (sr) return sr; }
        int rc = check_ready(d);
        if (rc) return rc;
        const bool geo_motion = compute_motion == 2;
        if (geo_motion && world != 1) return fail(ATN_ERR_UNSUPPORTED, "compute_motion = 2 on a screen shard: the geometry history has no node-wide form");
        if (geo_motion) {
            if (!path_pass) return fail(ATN_ERR_UNSUPPORTED, "compute_motion = 2 needs the frame's primary hits: atn_svgf_denoise has no path pass");
            if (!gm_on) return fail(ATN_ERR_INVALID_ARG, "compute_motion = 2 needs geometry motion tracking: atn_set_geometry_motion(ctx, 1)");
            // the ids and primary_position must belong to the same sample: every sample's bounce 0 overwrites the position of the pixels
            // that still sample, so with several samples the two planes would have to be captured per pixel and sample -- refused
            if (d->sample != 1) return fail(ATN_ERR_UNSUPPORTED, "compute_motion = 2 renders one sample per pixel (destination.sample must be 1)");
        }
        ATN_HIP(hipSetDevice(device));
        // Frames in flight (atn_set_frames_in_flight > 1): the path pass of frame f + 1 runs on the next bank's stream while
        // frame f is still being traced and filtered.  The path pass writes only its bank and slot (f + 1) % 2 of the
        // hand-over planes (G-buffer staging, primary positions, contributions), so all it waits for is the prepare pass
        // that consumed that slot two frames ago; the filter passes run on one filter stream, frame after frame, each
        // waiting for its own path pass.
        const bool pipelined = frames_in_flight > 1 && path_pass;
        if (!pipelined && frames_in_flight > 1) { rc = quiesce(); if (rc) return rc; }
        else if (w_or_h_changed(d->width, d->height)) { rc = quiesce(); if (rc) return rc; }
        if (pipelined && !sv_stream && !sv_handover_only) ATN_HIP(hipStreamCreateWithFlags(&sv_stream.h, hipStreamNonBlocking));
        if (pipelined && !sv_ev_prepare[0]) for (auto& e : sv_ev_prepare) ATN_HIP(hipEventCreateWithFlags(&e.h, hipEventDisableTiming));
        rc = begin_frame(*d, pipelined);
        if (rc) return rc;
        hipStream_t fs = (pipelined && sv_stream) ? sv_stream : stream;       // the stream the filter passes run on
        rc = svgf_ensure(d->width, d->height, want_stages);
        if (rc) return rc;
        if (!compute_motion && !sv_handover_only && (!sv_motion.is_set || sv_motion.count < (size_t)d->width * d->height))
            return fail(ATN_ERR_INVALID_ARG, "no motion/depth buffer: call atn_svgf_set_motion_depth or pass compute_motion = 1");
        const bool prof = d->profile != 0;
        PathBuffers pb = buffers(false);
        FrameParams fp = frame_params(*d);
        fp.break_on_terminate = 1;

        sv_mtx.advance(camera);
        const int32_t cur = sv_curr, prv = 1 - sv_curr;
        SvgfFrame sf{};
        sf.nd = sv_aov[cur][0].p; sf.am = sv_aov[cur][1].p; sf.cv = sv_cv[cur]; sf.mt = sv_aov[cur][3].p;
        sf.pnd = sv_aov[prv][0].p; sf.pam = sv_aov[prv][1].p; sf.pcv = sv_cv[prv]; sf.pmt = sv_aov[prv][3].p;
        sf.cv_out = sv_spare;
        sf.atrous[0] = sv_atrous[0].p; sf.atrous[1] = sv_atrous[1].p;
        const int32_t slot = sv_slot;
        sv_last_slot = slot;
        sf.tmp = sv_tmp.p; sf.motion = sv_motion.buf.p; sf.primary = sv_primary[slot].p; sf.contribs = sv_contribs[slot].p;
        sf.g_nd = path_pass ? sv_gnd[slot].p : nullptr; sf.g_am = path_pass ? sv_gam[slot].p : nullptr;
        sf.out = sv_out.p; sf.stages = want_stages ? sv_stages.p : nullptr;
        mat_mul(sv_mtx.V2C, sv_mtx.W2V, sf.w2c);
        mat_mul(sv_mtx.V2C, sv_mtx.prevW2V, sf.prev_w2c);
        sf.width = d->width; sf.height = d->height; sf.frame = d->frame; sf.atrous_iter_cnt = sv_atrous_iters;
        // Camera::ComputeScreenDistance (camera.h:216-221): tan of half the fov IN DEGREES, as the reference writes it
        sf.camera_distance = (float)d->height / (2.0f * std::tan(0.5f * camera.vfov));
        sf.compute_motion = geo_motion ? 0 : compute_motion;       // mode 2: k_motion_geometry writes the plane, the prepare pass leaves it
        if (geo_motion) ATN_HIP(gm_ids[slot].resize((size_t)d->width * d->height));
        gm_sv_ids[slot] = geo_motion;
        SvgfShade sv{};
        sv.nd = sv_gnd[slot].p; sv.am = sv_gam[slot].p; sv.primary = sf.primary;
        sv.w2c3[0] = sf.w2c[12]; sv.w2c3[1] = sf.w2c[13]; sv.w2c3[2] = sf.w2c[14]; sv.w2c3[3] = sf.w2c[15];

        if (path_pass) {
            if (pipelined && sv_prepare_recorded[slot]) ATN_HIP(hipStreamWaitEvent(stream, sv_ev_prepare[slot], 0));
            gm_capture = geo_motion ? gm_ids[slot].p : nullptr;
            rc = run_paths<true>(d, fp, false, prof, sv, sf);
            gm_capture = nullptr;
            if (rc) return rc;
            if (geo_motion) {
                // the plane's last reader is the previous frame's temporal pass on the filter stream (the slot event is recorded behind it)
                if (pipelined && sv_prepare_recorded[1 - slot]) ATN_HIP(hipStreamWaitEvent(stream, sv_ev_prepare[1 - slot], 0));
                rc = taa_before_write(stream);      // ... or the display tail of that frame (atn_taa_resolve, source 0)
                if (rc) return rc;
                MotionArgs ma{};
                ma.ids = gm_ids[slot].p; ma.pos = sf.primary; ma.motion = sf.motion;
                std::memcpy(ma.w2c, sf.w2c, sizeof(ma.w2c)); std::memcpy(ma.prev_w2c, sf.prev_w2c, sizeof(ma.prev_w2c));
                prof_begin(prof, ATN_K_SVGF_PREPARE);
                rc = gm_motion_pass(ma, d->width, d->height);
                prof_end(prof);
                if (rc) return rc;
            }
            if (pipelined) {
                rc = record_scene_read();       // (this bank's "path pass done": ev_gather, which the filter half waits for)
                if (rc) return rc;
            }
            sv_slot = 1 - sv_slot;      // (the next path pass fills the other slot)
        }
        sv_pass.sf = sf; sv_pass.fs = fs; sv_pass.slot = slot; sv_pass.cur = cur;
        sv_pass.pipelined = pipelined; sv_pass.path_pass = path_pass; sv_pass.prof = prof;
        return ATN_OK;
    }

    // The filter half: everything of OnRender from PrepareForDenoise on, over the planes the path half (or atn_svgf_upload) left, on
    // the frame's filter stream.  Needs the WHOLE frame in the hand-over planes: on a node that is shard 0 behind the gather.
    int svgf_filter_half(const atn_destination* d, atn_vec4* out_host, atn_vec4* stages_host)
    {
        SvgfFrame sf = sv_pass.sf;
        hipStream_t fs = sv_pass.fs;
        const int32_t slot = sv_pass.slot, cur = sv_pass.cur;
        const bool pipelined = sv_pass.pipelined, prof = sv_pass.prof;
        if (pipelined && sv_pass.path_pass) ATN_HIP(hipStreamWaitEvent(fs, ev_gather, 0));
        const dim3 gp((((d->width + 7) / 8) + 7) / 8 * 8, (d->height + 31) / 32), tp(256);     // x: multiple of 8 (XCD strips)
        int rc = taa_before_write(fs);      // the prepare pass overwrites the output and motion planes a display tail may still read
        if (rc) return rc;
        prof_begin(prof, ATN_K_SVGF_PREPARE, fs);
        hipLaunchKernelGGL(k_svgf_prepare, gp, tp, 0, fs, sf);
        prof_end(prof);
        if (d->frame > 0) {
            prof_begin(prof, ATN_K_SVGF_TEMPORAL, fs);
            hipLaunchKernelGGL(k_svgf_temporal, gp, tp, 0, fs, sf, 0.98f, 0.05f);
            if (sv_dilate_weight) {
                ATN_HIP(sv_weight.resize((size_t)d->width * d->height));
                hipLaunchKernelGGL(k_svgf_dilate_weight, gp, tp, 0, fs, sf, sv_weight.p);
                hipLaunchKernelGGL(k_svgf_store_weight, gp, tp, 0, fs, sf, (const float*)sv_weight.p);
            }
            prof_end(prof);
        }
        else if (sf.stages) {
            // frame 0: the temporal pass only re-puts the raw contribution (svgf.cpp:549-551)
            ATN_HIP(hipMemcpyAsync(sf.stages + (size_t)d->width * d->height, sf.stages, (size_t)d->width * d->height * sizeof(float4), hipMemcpyDeviceToDevice, fs));
        }
        // the slot is free again only now: k_svgf_temporal is the last reader of the hand-over planes (it re-reads
        // sf.contribs[slot]); recording this right behind k_svgf_prepare let frame f + 2's k_svgf_sample_end overwrite them
        if (pipelined) { ATN_HIP(hipEventRecord(sv_ev_prepare[slot], fs)); sv_prepare_recorded[slot] = true; }
        prof_begin(prof, ATN_K_SVGF_VARIANCE, fs);
        hipLaunchKernelGGL(k_svgf_variance, gp, tp, 0, fs, sf);
        prof_end(prof);
        std::swap(sv_cv[cur], sv_spare);        // the pass wrote the new colour+variance into the spare buffer
        sf.cv = sv_cv[cur]; sf.cv_out = sv_spare;
        for (int32_t i = 0; i < sv_atrous_iters; i++) {
            prof_begin(prof, ATN_K_SVGF_ATROUS, fs);
            if (env_atrous4) {
                // four pixels per thread (svgf.hpp, k_svgf_atrous4): the thread grid covers the 2 x 2 pixel GROUPS of pitch 2^i
                const int32_t s = 1 << i;
                const int32_t nx = ((d->width + 2 * s - 1) / (2 * s)) * s, ny = ((d->height + 2 * s - 1) / (2 * s)) * s;
                const dim3 g4((((nx + 7) / 8) + 7) / 8 * 8, (ny + 31) / 32);
                hipLaunchKernelGGL(k_svgf_atrous4, g4, tp, 0, fs, sf, i);
            }
            else hipLaunchKernelGGL(k_svgf_atrous, gp, tp, 0, fs, sf, i);
            prof_end(prof);
        }
        prof_begin(prof, ATN_K_SVGF_PREPARE, fs);
        hipLaunchKernelGGL(k_svgf_copy, gp, tp, 0, fs, sf);
        prof_end(prof);
        ATN_HIP(hipGetLastError());
        sv_curr = 1 - sv_curr;
        sv_frame_done = true; sv_last_fs = fs;

        const size_t n = (size_t)d->width * d->height;
        if (out_host) ATN_HIP(hipMemcpyAsync(out_host, sv_out.p, n * sizeof(float4), hipMemcpyDeviceToHost, fs));
        if (stages_host) ATN_HIP(hipMemcpyAsync(stages_host, sv_stages.p, 3 * n * sizeof(float4), hipMemcpyDeviceToHost, fs));
        if (out_host || stages_host) ATN_HIP(hipStreamSynchronize(fs));
        return ATN_OK;
    }

    // ------------------------------------------------------------------------------------------------
    // ReSTIR (aten::ReSTIRRenderer / idaten::ReSTIRPathTracing, device/restir.hpp): frame-persistent state = the two reservoir and
    // info sets (ReuseParams, restir_types.h:117-168), the AOVs, the motion/depth buffer and MatricesForRendering
    // ------------------------------------------------------------------------------------------------
    DevBuf<float4> rs_res[2][kRestirResPlanes], rs_info[2][kRestirInfoPlanes], rs_nd, rs_am, rs_motion_own, rs_vis, rs_stage;
    MotionDepth rs_motion;
    // rs_motion: the caller's motion/depth buffer (atn_restir_set_motion_depth); rs_motion_own: the one compute_motion fills
    DevBuf<float> rs_dims;
    int32_t rs_w = 0, rs_h = 0, rs_pos = 0, rs_last = 0;     // rs_pos: the current set of the next frame; rs_last: of the last frame
    int32_t rs_mode = 1, rs_candidates = 32, rs_capture = 0;
    bool rs_rendered = false;
    bool rs_captured = false, rs_last_own_motion = false;      // the last frame wrote the stage buffers / used rs_motion_own
    FrameFence rs_fence;        // the last frame's reuse passes are done with the sets (the next frame's shade waits for it)
    FrameMatrices rs_mtx;

    int restir_set_options(int32_t mode, int32_t n_candidates)
    {
        if (mode < 0 || mode > 3) return fail(ATN_ERR_INVALID_ARG, "ReSTIR mode must be 0 (initial candidates), 1 (temporal + spatial), 2 (spatial) or 3 (temporal)");
        if (n_candidates < 1 || n_candidates > 32) return fail(ATN_ERR_INVALID_ARG, "n_candidates must be in [1, 32]");
        rs_mode = mode; rs_candidates = n_candidates;
        return ATN_OK;
    }

    // forget the history: both sets are re-initialised by the next frame, the camera matrices start from the identity
    int restir_reset()
    {
        rs_w = 0; rs_h = 0; rs_pos = 0; rs_last = 0; rs_rendered = false; rs_captured = false;
        rs_mtx.reset_identity();
        return ATN_OK;
    }

    // Reservoir() / ReSTIRInfo() of a fresh ReuseParams: y = -1, M = 0, mtrl_idx = mesh_id = -1
    int restir_ensure(int32_t w, int32_t h)
    {
        const size_t n = (size_t)w * h;
        float neg1;
        { const int32_t m1 = -1; std::memcpy(&neg1, &m1, 4); }
        if (w != rs_w || h != rs_h) {
            for (int k = 0; k < 2; k++) {
                for (auto& b : rs_res[k]) { ATN_HIP(b.resize(n)); fill4(b.p, n, make_float4(0, 0, 0, 0)); }
                for (auto& b : rs_info[k]) { ATN_HIP(b.resize(n)); fill4(b.p, n, make_float4(0, 0, 0, 0)); }
                fill4(rs_res[k][0].p, n, make_float4(0.0F, 0.0F, neg1, 0.0F));
                fill4(rs_info[k][0].p, n, make_float4(0.0F, 0.0F, 0.0F, neg1));
                fill4(rs_info[k][3].p, n, make_float4(0.0F, neg1, 0.0F, 0.0F));
            }
            ATN_HIP(rs_nd.resize(n)); fill4(rs_nd.p, n, make_float4(0, 0, 0, 1));
            ATN_HIP(rs_am.resize(n)); fill4(rs_am.p, n, make_float4(0, 0, 0, 1));
            if (!rs_motion.is_set || rs_motion.count < n) { ATN_HIP(rs_motion.buf.resize(n)); rs_motion.is_set = false; rs_motion.count = 0; }
            rs_w = w; rs_h = h; rs_pos = 0; rs_last = 0;
        }
        ATN_HIP(rs_vis.resize(n_slots));
        if (rs_capture) { ATN_HIP(rs_stage.resize(6 * n)); ATN_HIP(rs_dims.resize(n)); }
        return ATN_OK;
    }

    // ≙ idaten::ReSTIRPathTracing::render + OnRender (src/libidaten/restir/restir.cpp:47-100, restir.cu:321-420), with the CPU
    // renderer's sample stream (docs/RESTIR.md): generate the path once, bounce 0 = ReSTIR shade + visibility + temporal (frame > 1)
    // + spatial + pixel colour, bounces >= 1 = the path tracer's own k_shade.
    int restir_render(const atn_destination* d, int32_t compute_motion, atn_vec4* out_host)
    {
        { const int sr = sph_refuse("the ReSTIR renderer does not trace sphere leaves"); if (sr) return sr; }
        int rc = check_ready(d);
        if (rc) return rc;
        if (d->sample != 1) return fail(ATN_ERR_UNSUPPORTED, "ReSTIR renders one sample per pixel (destination.sample must be 1)");
        if (world != 1) return fail(ATN_ERR_UNSUPPORTED, "ReSTIR needs the whole frame on one GPU (spatial reuse reads pixels of other shards)");
        if (regen_mode != 0) return fail(ATN_ERR_UNSUPPORTED, "ReSTIR runs the serial sample loop: switch path regeneration off (atn_set_regeneration(0))");
        if (shade_math_relaxed) return fail(ATN_ERR_UNSUPPORTED, "ReSTIR has no relaxed-math kernels: atn_set_shade_math(0)");
        if (d->count_stats) return fail(ATN_ERR_UNSUPPORTED, "ReSTIR frames do not count rays (count_stats must be 0)");
        if (scene.material_set >= kMsToon) return fail(ATN_ERR_UNSUPPORTED, "ReSTIR does not shade toon / stylised materials");
        const bool geo_motion = compute_motion == 2;
        if (geo_motion && !gm_on) return fail(ATN_ERR_INVALID_ARG, "compute_motion = 2 needs geometry motion tracking: atn_set_geometry_motion(ctx, 1)");
        ATN_HIP(hipSetDevice(device));
        if (frames_in_flight > 1 && (d->width != rs_w || d->height != rs_h)) { rc = quiesce(); if (rc) return rc; }
        rc = begin_frame(*d, frames_in_flight > 1);
        if (rc) return rc;
        rc = restir_ensure(d->width, d->height);
        if (rc) return rc;
        const size_t n = (size_t)d->width * d->height;
        if (!compute_motion && (!rs_motion.is_set || rs_motion.count < n))
            return fail(ATN_ERR_INVALID_ARG, "no motion/depth buffer: call atn_restir_set_motion_depth or pass compute_motion = 1");
        if (compute_motion) ATN_HIP(rs_motion_own.resize(n));
        if (geo_motion) ATN_HIP(gm_rs_ids.resize(n));
        gm_rs_has_ids = geo_motion;
        const bool prof = d->profile != 0;
        rs_mtx.advance(camera);

        auto [fp, pb, plan] = serial_frame(*d);
        const int32_t cur = rs_pos, oth = 1 - rs_pos;
        RestirArgs ra{};
        for (int k = 0; k < kRestirResPlanes; k++) { ra.cur.res[k] = rs_res[cur][k].p; ra.other.res[k] = rs_res[oth][k].p; }
        for (int k = 0; k < kRestirInfoPlanes; k++) { ra.cur.info[k] = rs_info[cur][k].p; ra.other.info[k] = rs_info[oth][k].p; }
        ra.nd = rs_nd.p; ra.am = rs_am.p; ra.motion = compute_motion ? rs_motion_own.p : rs_motion.buf.p; ra.vis = rs_vis.p;
        mat_mul(rs_mtx.V2C, rs_mtx.W2V, ra.w2c);
        mat_mul(rs_mtx.V2C, rs_mtx.prevW2V, ra.prev_w2c);
        for (int k = 0; k < 4; k++) ra.w2c3[k] = ra.w2c[12 + k];
        ra.n_candidates = rs_candidates;
        ra.stage_res = rs_capture ? rs_stage.p : nullptr;
        ra.dims = rs_capture ? rs_dims.p : nullptr;
        PathBuffers pb_vis = pb;        // the visibility rays add their (1, 1, 1) to rs_vis instead of the path's contribution
        pb_vis.contrib = rs_vis.p;

        const uint32_t g_slots = grid_for(n_slots), g_all = (n_slots + 255u) / 256u;
        ATN_HIP(hipMemsetAsync(counters.p, 0, (size_t)4 * counters_depth * 4, stream));
        prof_begin(prof, ATN_K_GEN);
        hipLaunchKernelGGL(k_gen_path, dim3(g_slots), dim3(256), 0, stream, pb, fp, camera, (const uint32_t*)seeds.p);
        prof_end(prof);
        for (int32_t b = 0; b <= d->maxDepth; b++) {
            const TraceLaunch tl = trace_launch(plan, b);
            prof_begin(prof, tl.prof_kind);
            launch_trace_fused<false>(tl, stream, b == 1 ? pb_vis : pb, scene, b - 1, b < d->maxDepth ? b : -1, b);
            prof_end(prof);
            if (b == 1) {
                // EvaluateVisibility's outcome, ApplyTemporalReuse (frame > 1), ApplySpatialReuse + ComputePixelColor (ReSTIRMode,
                // restir.h:25-29; restir_reuse.cpp:132-213)
                const bool temporal = (rs_mode == 1 || rs_mode == 3) && d->frame > 1;
                prof_begin(prof, ATN_K_SHADE);
                restir_launch_temporal(scene.material_set, temporal, stream, pb, scene, fp, ra);
                if (rs_mode == 1 || rs_mode == 2) restir_launch_spatial(scene.material_set, stream, pb, scene, fp, ra);
                else restir_launch_color(scene.material_set, stream, pb, scene, fp, ra);
                prof_end(prof);
                ATN_HIP(rs_fence.record(stream));
            }
            if (b == d->maxDepth) break;
            prof_begin(prof, ATN_K_SHADE);
            if (b == 0) {
                // the previous frame's reuse passes read the sets, AOVs and visibility plane this frame's bounce 0 overwrites
                if (frames_in_flight > 1) ATN_HIP(rs_fence.wait(stream));
                rc = taa_before_write(stream);      // (the motion plane a display tail may still read: atn_taa_resolve, source 1)
                if (rc) return rc;
                restir_launch_shade(scene.material_set, plan.shade_grid, stream, pb, scene, fp, camera, ra);
                if (geo_motion) {
                    // (the hit records of bounce 0 stay in the path state until the next trace launch)
                    motion_launch_capture(g_all, stream, pb, fp, gm_rs_ids.p);
                    MotionArgs ma{};
                    ma.ids = gm_rs_ids.p; ma.pos = ra.cur.info[2]; ma.motion = ra.motion;
                    std::memcpy(ma.w2c, ra.w2c, sizeof(ma.w2c)); std::memcpy(ma.prev_w2c, ra.prev_w2c, sizeof(ma.prev_w2c));
                    rc = gm_motion_pass(ma, d->width, d->height);
                    if (rc) return rc;
                }
                else if (compute_motion) restir_launch_motion(stream, fp, ra);
                restir_launch_vis_prep(grid_for(n_slots), stream, pb, scene, fp, ra);
            }
            else launch_shade<false>(plan, stream, pb, fp, b, SvgfShade{});
            prof_end(prof);
        }
        rs_last = cur;
        rs_pos = oth;           // ReuseParams::Update, every frame whatever the mode
        rs_rendered = true;
        rs_captured = rs_capture != 0;
        rs_last_own_motion = compute_motion != 0;
        rc = gather_film(*d, pb, fp);       // (one sample per pixel: k_gather<true>)
        return rc ? rc : end_film_frame(*d, out_host);
    }

    // stage buffers of the last frame (tests): 0 / 1 / 2 the reservoirs after the shade, temporal (visibility) and spatial passes as
    // float[n][5] {y, M, W, w_sum, target_pdf_of_y} (atn_restir_capture); 3 the infos float4[4][n]; 4 / 5 the AOVs; 6 motion-depth;
    // 7 the CMJ dimension of every pixel after bounce 0's passes, uint32[n] (atn_restir_capture); 8 the ids plane of a frame rendered
    // with compute_motion = 2 (device/motion.hpp)
    int restir_download(int32_t which, void* out)
    {
        if (!rs_rendered || !out) return fail(ATN_ERR_INVALID_ARG, "no ReSTIR frame has been rendered");
        const size_t n = (size_t)rs_w * rs_h;
        { const int s = settle(); if (s) return s; }
        if ((which <= 2 || which == 7) && !rs_captured) return fail(ATN_ERR_INVALID_ARG, "the last frame kept no stage buffers: atn_restir_capture(ctx, 1) before the frame");
        if (which >= 0 && which <= 2) {
            std::vector<float4> h(2 * n);
            ATN_HIP(hipMemcpy(h.data(), rs_stage.p + (size_t)which * 2 * n, 2 * n * sizeof(float4), hipMemcpyDeviceToHost));
            float* o = static_cast<float*>(out);
            for (size_t i = 0; i < n; i++) {
                const float4 a = h[i], b = h[n + i];
                int32_t y, M;
                std::memcpy(&M, &a.y, 4); std::memcpy(&y, &a.z, 4);
                o[5 * i] = (float)y; o[5 * i + 1] = (float)M; o[5 * i + 2] = a.w; o[5 * i + 3] = a.x; o[5 * i + 4] = b.x;
            }
            return ATN_OK;
        }
        if (which == 3) {
            for (int k = 0; k < kRestirInfoPlanes; k++)
                ATN_HIP(hipMemcpy(static_cast<float4*>(out) + (size_t)k * n, rs_info[rs_last][k].p, n * sizeof(float4), hipMemcpyDeviceToHost));
            return ATN_OK;
        }
        const void* src = which == 4 ? (const void*)rs_nd.p : which == 5 ? (const void*)rs_am.p : which == 6 ? (const void*)(rs_last_own_motion ? rs_motion_own.p : rs_motion.buf.p)
                        : which == 7 ? (const void*)rs_dims.p : (which == 8 && gm_rs_has_ids) ? (const void*)gm_rs_ids.p : nullptr;
        if (!src) return fail(ATN_ERR_INVALID_ARG, "no such ReSTIR buffer");
        if (which == 7) {
            std::vector<float> h(n);
            ATN_HIP(hipMemcpy(h.data(), src, n * sizeof(float), hipMemcpyDeviceToHost));
            for (size_t i = 0; i < n; i++) static_cast<uint32_t*>(out)[i] = (uint32_t)h[i];
            return ATN_OK;
        }
        ATN_HIP(hipMemcpy(out, src, n * sizeof(float4), hipMemcpyDeviceToHost));
        return ATN_OK;
    }

    // ------------------------------------------------------------------------------------------------
    // The display tail (aten::TAA + aten::GammaCorrection, device/taa.hpp; docs/TAA.md): frame-persistent state = the history ping-pong
    // (taa.cpp:33-60).  One launch per frame, enqueued on the stream that produced its source and ordered against the next frame's
    // writers by ta_fence (taa_before_write).
    // ------------------------------------------------------------------------------------------------
    DevBuf<float4> ta_hist[2], ta_gamma, ta_up_color, ta_up_motion;
    DevBuf<uint32_t> ta_rgba8;
    int32_t ta_w = 0, ta_h = 0, ta_pos = 0;         // ta_hist[ta_pos]: the last output = the history of the next frame
    int32_t ta_up_w[2] = { 0, 0 }, ta_up_h[2] = { 0, 0 };       // sizes of the uploaded colour / motion planes (source 2)
    bool ta_valid = false;          // a history exists (false: the next frame takes the pass-through rule for every pixel)
    bool ta_resolved = false, ta_has_gamma = false;     // a frame has been resolved at ta_w x ta_h / and it wrote the float gamma plane
    FrameFence ta_fence;        // the last display tail has finished (its reads of the source planes and of the history)
    hipStream_t ta_last_stream = nullptr;
    static constexpr int32_t kTaaMaxSide = 16384;

    // in front of a pass that overwrites a plane the last display tail reads
    int taa_before_write(hipStream_t st)
    {
        ATN_HIP(ta_fence.wait(st));
        return ATN_OK;
    }
    int taa_idle()
    {
        if (ta_fence.pending) { ATN_HIP(hipStreamSynchronize(ta_last_stream)); ta_fence.pending = false; }
        return ATN_OK;
    }
    // a size change forgets the history
    int taa_ensure(int32_t w, int32_t h)
    {
        if (w <= 0 || h <= 0 || w > kTaaMaxSide || h > kTaaMaxSide) return fail(ATN_ERR_INVALID_ARG, "TAA: bad frame size (1 .. 16384 per side)");
        if (w == ta_w && h == ta_h) return ATN_OK;
        const int rc = taa_idle();
        if (rc) return rc;
        const size_t n = (size_t)w * h;
        for (auto& b : ta_hist) ATN_HIP(b.resize(n));
        ATN_HIP(ta_rgba8.resize(n));
        ta_w = w; ta_h = h; ta_pos = 0;
        ta_valid = false; ta_resolved = false; ta_has_gamma = false;
        return ATN_OK;
    }
    int taa_reset()
    {
        ta_valid = false;
        return ATN_OK;
    }
    // which: 0 the colour, 1 the motion/depth plane (source 2 of taa_resolve), 2 the history
    int taa_upload(int32_t which, int32_t w, int32_t h, const atn_vec4* host)
    {
        if (!host || which < 0 || which > 2) return fail(ATN_ERR_INVALID_ARG, "atn_taa_upload: which = 0 colour, 1 motion/depth, 2 history; host must not be null");
        if (w <= 0 || h <= 0 || w > kTaaMaxSide || h > kTaaMaxSide) return fail(ATN_ERR_INVALID_ARG, "TAA: bad frame size (1 .. 16384 per side)");
        ATN_HIP(hipSetDevice(device));
        int rc = taa_idle();
        if (rc) return rc;
        const size_t n = (size_t)w * h;
        float4* dst;
        if (which == 2) {
            rc = taa_ensure(w, h);
            if (rc) return rc;
            dst = ta_hist[ta_pos].p;
        }
        else {
            DevBuf<float4>& b = which == 0 ? ta_up_color : ta_up_motion;
            ATN_HIP(b.resize(n));
            dst = b.p;
        }
        ATN_HIP(hipMemcpyAsync(dst, host, n * sizeof(float4), hipMemcpyHostToDevice, stream));
        ATN_HIP(hipStreamSynchronize(stream));
        if (which == 2) ta_valid = true;
        else { ta_up_w[which] = w; ta_up_h[which] = h; }
        return ATN_OK;
    }
    // which: 0 the TAA output (= the new history), 1 the history the last frame read, 2 the gamma plane as float4, 3 as RGBA8
    int taa_download(int32_t which, void* out)
    {
        if (!out || which < 0 || which > 3) return fail(ATN_ERR_INVALID_ARG, "atn_taa_download: which = 0 output, 1 previous history, 2 gamma float, 3 gamma RGBA8; out must not be null");
        if (!ta_resolved) return fail(ATN_ERR_INVALID_ARG, "atn_taa_download: atn_taa_resolve has not run (at this size)");
        if (which == 2 && !ta_has_gamma) return fail(ATN_ERR_INVALID_ARG, "atn_taa_download: the last atn_taa_resolve did not ask for the float gamma plane");
        ATN_HIP(hipSetDevice(device));
        const int rc = taa_idle();
        if (rc) return rc;
        const size_t n = (size_t)ta_w * ta_h;
        const void* src = which == 0 ? (const void*)ta_hist[ta_pos].p : which == 1 ? (const void*)ta_hist[1 - ta_pos].p
                        : which == 2 ? (const void*)ta_gamma.p : (const void*)ta_rgba8.p;
        ATN_HIP(hipMemcpy(out, src, n * (which == 3 ? sizeof(uint32_t) : sizeof(float4)), hipMemcpyDeviceToHost));
        return ATN_OK;
    }
    // ≙ TAA::prePostProc / postPostProc around the fragment shader (taa.cpp:33-60) + GammaCorrection
    int taa_resolve(int32_t source, int32_t w, int32_t h, int32_t enable, float gamma, atn_vec4* out_f, uint32_t* out_8)
    {
        if (!(gamma > 0.0F) || !std::isfinite(gamma)) return fail(ATN_ERR_INVALID_ARG, "atn_taa_resolve: gamma must be finite and > 0");
        if (w <= 0 || h <= 0 || w > kTaaMaxSide || h > kTaaMaxSide) return fail(ATN_ERR_INVALID_ARG, "TAA: bad frame size (1 .. 16384 per side)");
        ATN_HIP(hipSetDevice(device));
        TaaArgs a{};
        hipStream_t st = stream;
        switch (source) {
        case 0:
            if (!sv_frame_done) return fail(ATN_ERR_INVALID_ARG, "atn_taa_resolve: source 0 needs an atn_svgf_render / atn_svgf_denoise frame");
            if (w != sv_w || h != sv_h) return fail(ATN_ERR_INVALID_ARG, "atn_taa_resolve: the last SVGF frame has another size");
            a.cur = sv_out.p; a.motion = sv_motion.buf.p; st = sv_last_fs;
            break;
        case 1:
            if (!rs_rendered) return fail(ATN_ERR_INVALID_ARG, "atn_taa_resolve: source 1 needs an atn_restir_render frame");
            if (w != rs_w || h != rs_h || w != film_w || h != film_h) return fail(ATN_ERR_INVALID_ARG, "atn_taa_resolve: the last ReSTIR frame has another size");
            a.cur = film.p; a.motion = rs_last_own_motion ? rs_motion_own.p : rs_motion.buf.p;      // (the frame's film writer ran on `stream`)
            break;
        case 2:
            if (ta_up_w[0] != w || ta_up_h[0] != h || ta_up_w[1] != w || ta_up_h[1] != h)
                return fail(ATN_ERR_INVALID_ARG, "atn_taa_resolve: source 2 needs atn_taa_upload of the colour and the motion/depth plane at this size");
            a.cur = ta_up_color.p; a.motion = ta_up_motion.p;
            break;
        default:
            return fail(ATN_ERR_INVALID_ARG, "atn_taa_resolve: source 0 (SVGF), 1 (ReSTIR) or 2 (uploaded planes)");
        }
        int rc = taa_ensure(w, h);
        if (rc) return rc;
        const size_t n = (size_t)w * h;
        if (out_f && ta_gamma.n < n) {
            rc = taa_idle();
            if (rc) return rc;
            ATN_HIP(ta_gamma.resize(n));
        }
        // behind the previous display tail (it wrote this frame's history), whatever stream that ran on
        if (ta_last_stream != st) ATN_HIP(ta_fence.wait(st));
        a.hist = ta_hist[ta_pos].p; a.out = ta_hist[1 - ta_pos].p;
        a.gamma_f = out_f ? ta_gamma.p : nullptr; a.rgba8 = ta_rgba8.p;
        a.width = w; a.height = h;
        a.enable = (enable != 0 && ta_valid) ? 1 : 0;       // no history: the frame passes through (docs/TAA.md, first frame)
        a.inv_gamma = 1.0F / gamma;
        taa_launch_resolve(tile_launch(w, h), st, a);
        ATN_HIP(hipGetLastError());
        ATN_HIP(ta_fence.record(st));
        ta_last_stream = st;
        ta_pos = 1 - ta_pos;
        ta_valid = true; ta_resolved = true; ta_has_gamma = out_f != nullptr;
        if (out_f) ATN_HIP(hipMemcpyAsync(out_f, ta_gamma.p, n * sizeof(float4), hipMemcpyDeviceToHost, st));
        if (out_8) ATN_HIP(hipMemcpyAsync(out_8, ta_rgba8.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        if (out_f || out_8) ATN_HIP(hipStreamSynchronize(st));
        return ATN_OK;
    }

    // ------------------------------------------------------------------------------------------------
    // NPR feature lines (aten::NprPathTracer::radiance_with_feature_line / idaten::NPRPathTracing, device/npr.hpp; docs/NPR.md):
    // per-slot sample-ray state, the bounce's ray list, and what the upload decoded of FeatureLineConfig / FeatureLineMtrlConfig
    // (read by the NPR kernels only)
    // ------------------------------------------------------------------------------------------------
    DevBuf<float4> np_disc_c, np_disc_n, np_desc_p, np_desc_n, np_ray_o, np_ray_d, np_ray_hit, np_st_line, np_st_desc, np_st_disc;
    DevBuf<uint32_t> np_live, np_work, np_counters, np_queue, np_mflags, np_st_dims;
    DevBuf<float> np_hpd;
    std::vector<uint32_t> np_mflags_host;
    atn_feature_line_config np_cfg{};
    bool np_stencil = false, np_alpha = false, np_carpaint = false;     // what the refusals need (upload, edits)
    bool maybe_alpha = false;       // a material has kAttrMaybeAlpha (np_alpha / vl_alpha = that and the config's enable_alpha_blending)
    uint32_t np_slots = 0;
    int32_t np_w = 0, np_h = 0, np_capture = 0, np_depth = 0;
    bool np_captured = false;
    FrameFence np_fence;        // the last NPR frame's kernels are done with the sample-ray state (the next frame waits for it)
    // the look-through (atn_npr_set_skip_through(1), device/npr_advance.hpp; docs/NPR_ADVANCE.md): the alpha-blend plane, the check's
    // working ray and record per slot, the queue without the paths whose look-through missed; shared by the banks like the state above
    int32_t np_skip = 0;
    DevBuf<float4> np_ab, np_adv_o, np_adv_d, np_st_adv;
    DevBuf<uint32_t> np_ab_acc, np_adv_info, np_adv_queue, np_adv_counters;
    uint32_t np_adv_slots = 0;
    int32_t np_adv_depth = 0;
    bool np_adv_captured = false;
    // does an NPR frame of the uploaded scene look through surfaces?  (a STENCIL material, or alpha blending with an alpha that may be < 1)
    bool npr_advances() const { return np_skip == 1 && (np_stencil || np_alpha); }
    int npr_set_skip_through(int32_t mode)
    {
        if (mode != 0 && mode != 1) return fail(ATN_ERR_INVALID_ARG, "NPR skip-through: mode is 0 (such scenes are refused) or 1 (AdvanceNPRPath)");
        np_skip = mode;
        return ATN_OK;
    }
    int npr_adv_ensure(int32_t w, int32_t h, int32_t max_depth)
    {
        if (n_slots != np_adv_slots) {
            ATN_HIP(np_ab.resize(n_slots)); ATN_HIP(np_adv_o.resize(n_slots)); ATN_HIP(np_adv_d.resize(n_slots));
            ATN_HIP(np_ab_acc.resize(n_slots)); ATN_HIP(np_adv_info.resize(n_slots)); ATN_HIP(np_adv_queue.resize(n_slots));
            np_adv_slots = n_slots;
        }
        if (max_depth > np_adv_depth) { ATN_HIP(np_adv_counters.resize((size_t)kAdvCounters * max_depth)); np_adv_depth = max_depth; }
        if (np_capture) ATN_HIP(np_st_adv.resize(2 * (size_t)w * h));
        return ATN_OK;
    }

    // (of src, the editable scene data as last uploaded or edited; `mats` = the device form of src.materials)
    int npr_decode(const std::vector<DevMaterial>& mats)
    {
        std::memcpy(&np_cfg, src.config.feature_line, sizeof(np_cfg));
        const size_t nm = src.materials.size();
        np_mflags_host.assign(nm + 1, 0u);        // (+ the white-diffuse fallback: no lines)
        np_stencil = false; np_carpaint = false;
        bool any_shadow = false;
        for (size_t i = 0; i < nm; i++) {
            const atn_material_param& m = src.materials[i];
            atn_feature_line_mtrl fl;
            std::memcpy(&fl, m.feature_line, sizeof(fl));
            np_mflags_host[i] = (fl.enable ? 1u : 0u) | ((uint32_t)fl.metric_flag << 8);
            if (m.stencil_type == 2) np_stencil = true;         // StencilType::STENCIL
            if (m.type == ATN_MTRL_CARPAINT) np_carpaint = true;
            if ((m.type == ATN_MTRL_TOON || m.type == ATN_MTRL_STYLIZED_BRDF) && m.toon.stylized_shadow.enable) any_shadow = true;
        }
        ns_any = any_shadow;
        maybe_alpha = false;
        for (const DevMaterial& dm : mats) if (dm.attrib & kAttrMaybeAlpha) maybe_alpha = true;
        np_alpha = src.config.enable_alpha_blending != 0 && maybe_alpha;
        ATN_HIP(np_mflags.upload(np_mflags_host, stream));
        return ATN_OK;
    }

    // the per-slot state: previous hit points and normals start at zero (SampleRayInfo's vec3s) and persist across samples and frames
    int npr_ensure(int32_t w, int32_t h, int32_t max_depth)
    {
        if (n_slots != np_slots) {
            const size_t r = (size_t)kNprRays * n_slots;
            if (r >= ((size_t)1 << 28)) return fail(ATN_ERR_UNSUPPORTED, "NPR frames list at most 2^28 sample rays per bounce (shard the screen)");
            ATN_HIP(np_disc_c.resize(n_slots)); ATN_HIP(np_disc_n.resize(n_slots));
            ATN_HIP(np_desc_p.resize(r)); ATN_HIP(np_desc_n.resize(r));
            ATN_HIP(np_ray_o.resize(r)); ATN_HIP(np_ray_d.resize(r)); ATN_HIP(np_ray_hit.resize(r));
            ATN_HIP(np_live.resize(n_slots)); ATN_HIP(np_work.resize(n_slots)); ATN_HIP(np_hpd.resize(n_slots)); ATN_HIP(np_queue.resize(n_slots));
            ATN_HIP(hipMemsetAsync(np_desc_p.p, 0, r * sizeof(float4), stream));
            ATN_HIP(hipMemsetAsync(np_desc_n.p, 0, r * sizeof(float4), stream));
            np_slots = n_slots;
        }
        if (max_depth > np_depth) { ATN_HIP(np_counters.resize((size_t)kNprCounters * max_depth)); np_depth = max_depth; }
        if (np_capture) {
            const size_t n = (size_t)w * h;
            ATN_HIP(np_st_line.resize(n)); ATN_HIP(np_st_desc.resize(kNprRays * n)); ATN_HIP(np_st_disc.resize(2 * n)); ATN_HIP(np_st_dims.resize(n));
        }
        np_w = w; np_h = h;
        return ATN_OK;
    }

    // Camera::ComputePixelWidthAtDistance (camera.h:182-197): the "hfov" is vfov * H / W, in degrees
    static float pixel_width_at(const atn_camera_param& c, float d)
    {
        d = std::fabs(d);
        float hfov = c.vfov * c.height / float(c.width);
        hfov = 3.14159265358979323846F * hfov / 180.0F;
        const float half = std::tan(hfov / 2) * d;
        return (half * 2) / float(c.width);
    }

    // ≙ NPRPathTracing::OnRender = PathTracing::OnRender with the hooks of npr_pathtracing.cu:388-517, the per-path arithmetic of the
    // CPU renderer (npr.cpp:101-200): one pass of the sample loop per frame (docs/NPR.md)
    int npr_render(const atn_destination* d, atn_vec4* out_host)
    {
        { const int sr = sph_refuse("the NPR renderer does not trace sphere leaves"); if (sr) return sr; }
        int rc = check_ready(d);
        if (rc) return rc;
        if (!np_cfg.enabled) return fail(ATN_ERR_UNSUPPORTED, "feature lines are off in the scene's config (FeatureLineConfig.enabled == 0): render with atn_render");
        if (np_stencil && np_skip != 1) return fail(ATN_ERR_UNSUPPORTED, "NPR frames do not skip through StencilType::STENCIL materials (AdvanceNPRPath)");
        if (np_alpha && np_skip != 1) return fail(ATN_ERR_UNSUPPORTED, "NPR frames do not skip through translucent-by-alpha surfaces: alpha blending is on and a material's alpha may be < 1 (AdvanceNPRPath)");
        if (np_carpaint) return fail(ATN_ERR_UNSUPPORTED, "NPR frames do not draw AdvanceNPRPath's extra CarPaint dimension: CarPaint materials are refused");
        if (world != 1) return fail(ATN_ERR_UNSUPPORTED, "NPR frames need the whole frame on one GPU (atn_set_screen_shard world 1)");
        if (regen_mode != 0) return fail(ATN_ERR_UNSUPPORTED, "NPR frames run the serial sample loop: switch path regeneration off (atn_set_regeneration(0))");
        if (shade_math_relaxed) return fail(ATN_ERR_UNSUPPORTED, "NPR frames have no relaxed-math kernels: atn_set_shade_math(0)");
        if (d->count_stats) return fail(ATN_ERR_UNSUPPORTED, "NPR frames do not count rays (count_stats must be 0)");
        // the pre-pass has a primary pass of its own, which would need the same look-through
        const bool adv = npr_advances();
        if (adv && ns_mode == 1 && (nh_base != 1 || nh_dir != kHatchHorizontal))
            return fail(ATN_ERR_UNSUPPORTED, "NPR skip-through: the hatching pre-pass does not look through STENCIL or alpha surfaces: atn_npr_hatching_set(1, 1, ...) and atn_npr_shadow_set_mode(0), or atn_npr_set_skip_through(0)");
        if (adv && ns_mode == 1)
            return fail(ATN_ERR_UNSUPPORTED, "NPR skip-through: the shadow pre-pass does not look through STENCIL or alpha surfaces: atn_npr_shadow_set_mode(0), or atn_npr_set_skip_through(0)");
        rc = nh_check(d);
        if (rc) return rc;
        ATN_HIP(hipSetDevice(device));
        rc = begin_frame(*d, frames_in_flight > 1);
        if (rc) return rc;
        rc = npr_ensure(d->width, d->height, d->maxDepth);
        if (rc) return rc;
        if (adv) { rc = npr_adv_ensure(d->width, d->height, d->maxDepth); if (rc) return rc; }
        // atn_npr_shadow_set_mode(1): the same pre-pass as with lines off (docs/NPR_SHADOW.md)
        if (ns_frame()) { rc = ns_prepass(d); if (rc) return rc; }
        const bool prof = d->profile != 0;
        auto [fp, pb, plan] = serial_frame(*d);
        NprArgs na{};
        na.disc_c = np_disc_c.p; na.disc_n = np_disc_n.p; na.desc_p = np_desc_p.p; na.desc_n = np_desc_n.p;
        na.live = np_live.p; na.work = np_work.p; na.hpd = np_hpd.p;
        na.ray_o = np_ray_o.p; na.ray_d = np_ray_d.p; na.ray_hit = np_ray_hit.p;
        na.counters = np_counters.p; na.queue = np_queue.p; na.mflags = np_mflags.p;
        for (int k = 0; k < 3; k++) na.line_color[k] = np_cfg.line_color[k];
        na.line_width = np_cfg.line_width; na.albedo_threshold = np_cfg.albedo_threshold; na.normal_threshold = np_cfg.normal_threshold;
        na.pixel_width = pixel_width_at(camera, 1.0F);
        if (np_capture) { na.st_line = np_st_line.p; na.st_desc = np_st_desc.p; na.st_disc = np_st_disc.p; na.st_dims = np_st_dims.p; }
        // the walk of the sample rays: the frame's walk, LDS copy and block, 8 rays per path
        const RayLaunch nl = ray_launch(plan, n_slots, kNprRays * n_slots, trace_grid(kNprRays * n_slots, true));
        // the look-through's walk: one job per path
        NprAdvArgs aa{};
        RayLaunch al{};
        if (adv) {
            aa.queue_in = np_queue.p; aa.counters_in = np_counters.p; aa.queue_out = np_adv_queue.p; aa.counters = np_adv_counters.p;
            aa.ab = np_ab.p; aa.ab_acc = np_ab_acc.p; aa.ray_o = np_adv_o.p; aa.ray_d = np_adv_d.p; aa.info = np_adv_info.p;
            aa.st_adv = np_capture ? np_st_adv.p : nullptr;
            aa.max_depth = d->maxDepth;
            al = ray_launch(plan, n_slots, n_slots, trace_grid(n_slots, true));
        }

        const uint32_t g_slots = grid_for(n_slots), g_all = (n_slots + 255u) / 256u;
        // the previous NPR frame (another bank's stream) still reads and writes the sample-ray state
        if (frames_in_flight > 1) ATN_HIP(np_fence.wait(stream));
        if (np_capture) ATN_HIP(hipMemsetAsync(np_st_line.p, 0, (size_t)d->width * d->height * sizeof(float4), stream));
        ATN_HIP(hipMemsetAsync(counters.p, 0, (size_t)4 * counters_depth * 4, stream));
        for (int32_t s = 0; s < d->sample; s++) {
            fp.sample = s;
            if (s > 0) ATN_HIP(hipMemsetAsync(pb.q_count, 0, (size_t)4 * counters_depth * 4, stream));
            ATN_HIP(hipMemsetAsync(np_counters.p, 0, (size_t)kNprCounters * d->maxDepth * sizeof(uint32_t), stream));
            prof_begin(prof, ATN_K_GEN);
            hipLaunchKernelGGL(k_gen_path, dim3(g_slots), dim3(256), 0, stream, pb, fp, camera, (const uint32_t*)seeds.p);
            npr_launch_gen(g_slots, stream, pb, fp, na);
            if (adv) {
                ATN_HIP(hipMemsetAsync(np_adv_counters.p, 0, (size_t)kAdvCounters * d->maxDepth * sizeof(uint32_t), stream));
                npr_adv_launch_init(g_all, stream, fp, aa);
            }
            prof_end(prof);
            for (int32_t b = 0; b <= d->maxDepth; b++) {
                const TraceLaunch tl = trace_launch(plan, b);
                prof_begin(prof, tl.prof_kind);
                launch_trace_fused<false>(tl, stream, pb, scene, b - 1, b < d->maxDepth ? b : -1, b);
                prof_end(prof);
                if (b == d->maxDepth) break;
                // prep, the sample rays' walk, eval: the paths a line ended leave the queue k_shade reads
                npr_launch_bounce(nl, stream, pb, scene, fp, camera, na, b);
                PathBuffers pbs = pb;
                pbs.queue[b & 1] = np_queue.p;
                if (adv) {
                    // AdvanceNPRPath: the paths that look through a surface get their new hit and ray; those that end in a miss leave
                    // this bounce's shade queue for the next bounce's trace queue
                    prof_begin(prof, ATN_K_TRACE_FUSED);
                    npr_adv_launch_bounce(al, stream, pb, scene, aa, b);
                    prof_end(prof);
                    if (b == 0 && np_capture) npr_adv_launch_capture0(g_all, stream, pb, fp, aa);
                    pbs.queue[b & 1] = np_adv_queue.p;
                    prof_begin(prof, ATN_K_SHADE);
                    if (npr_adv_launch_shade(scene.material_set, plan.shade_waves, plan.shade_grid, stream, pbs, scene, fp, camera, b, np_ab.p))
                        return fail(ATN_ERR_UNSUPPORTED, "NPR skip-through: no alpha-blend shade kernel for the scene's material set");
                    prof_end(prof);
                }
                else {
                    prof_begin(prof, ATN_K_SHADE);
                    launch_shade<false>(plan, stream, pbs, fp, b, SvgfShade{});
                    prof_end(prof);
                }
                if (b == 0 && np_capture) npr_launch_capture0(g_all, stream, pb, fp, na);
            }
            if (d->sample > 1) {
                prof_begin(prof, ATN_K_ACCUM);
                hipLaunchKernelGGL(k_accumulate_sample, dim3(g_all), dim3(256), 0, stream, pb, fp);
                prof_end(prof);
            }
        }
        ATN_HIP(np_fence.record(stream));
        np_captured = np_capture != 0;
        np_adv_captured = np_captured && adv;
        rc = ns_end_frame();
        if (rc) return rc;
        rc = gather_film(*d, pb, fp);
        return rc ? rc : end_film_frame(*d, out_host);
    }

    // the film and the sample-ray state of a fresh context
    int npr_reset()
    {
        ATN_HIP(hipSetDevice(device));
        { int q = quiesce(); if (q) return q; }
        if (np_desc_p.p) {
            ATN_HIP(hipMemsetAsync(np_desc_p.p, 0, np_desc_p.n * sizeof(float4), stream));
            ATN_HIP(hipMemsetAsync(np_desc_n.p, 0, np_desc_n.n * sizeof(float4), stream));
        }
        np_captured = false; np_adv_captured = false;
        return reset();
    }

    int npr_advance_download(void* out)
    {
        if (!out) return fail(ATN_ERR_INVALID_ARG, "null output");
        if (!np_adv_captured) return fail(ATN_ERR_INVALID_ARG, "the last NPR frame kept no look-through stage: atn_npr_capture(ctx, 1) and atn_npr_set_skip_through(ctx, 1) before a frame of a scene that needs it");
        const StageBuf bufs[] = { { np_st_adv.p, 2 * (size_t)np_w * np_h * sizeof(float4) } };
        return download_stage(bufs, 0, out, "no such NPR buffer");
    }

    int npr_download(int32_t which, void* out)
    {
        if (!out) return fail(ATN_ERR_INVALID_ARG, "null output");
        if (!np_captured) return fail(ATN_ERR_INVALID_ARG, "the last NPR frame kept no stage buffers: atn_npr_capture(ctx, 1) before the frame");
        const size_t n = (size_t)np_w * np_h;
        const StageBuf bufs[] = { { np_st_line.p, n * sizeof(float4) }, { np_st_desc.p, kNprRays * n * sizeof(float4) },
                                  { np_st_disc.p, 2 * n * sizeof(float4) }, { np_st_dims.p, n * sizeof(uint32_t) } };
        return download_stage(bufs, which, out, "no such NPR buffer");
    }

    // ------------------------------------------------------------------------------------------------
    // Volume rendering (aten::VolumePathTracing::radiance / Nee, device/volume.hpp; docs/VOLUME.md): per-slot medium stack and
    // connection records, and what the upload decoded of is_medium / type / MediumParameter (read by the volume kernels only)
    // ------------------------------------------------------------------------------------------------
    DevBuf<VolMedium> vl_med;
    DevBuf<uint4> vl_stack, vl_c_stack, vl_st_state, vl_st_stack;
    DevBuf<uint32_t> vl_meta, vl_conn_q, vl_counters;
    DevBuf<float> vl_hit_t;
    DevBuf<float4> vl_ev_o, vl_ev_d, vl_c_o, vl_c_d, vl_c_w, vl_c_a, vl_c_b, vl_c_c, vl_st_ray, vl_st_conn;
    DevBuf<uint2> vl_segs;
    std::string vl_refuse;          // why the uploaded scene's media cannot be rendered ("" = they can)
    bool vl_stencil = false, vl_alpha = false, vl_carpaint = false, vl_toon = false;
    float vl_eps_bias = 0.0F;
    int32_t vl_w = 0, vl_h = 0, vl_capture = -1, vl_captured = -1;
    bool vl_rendered = false;
    FrameFence vl_fence;        // the last volume frame's kernels are done with the per-slot state (the next frame waits for it)
    // Grid media (atn_volume_set_grids; device/volume_grid.hpp): dense float grids a medium material names by grid_idx.  They outlive
    // atn_update_*; atn_upload_scene drops them.  What is wrong with a grid, or with a material that names one, is kept as a
    // message and refused by atn_volume_render.
    struct VolGridHost {
        int32_t dim[3] = { 0, 0, 0 };
        float max_density = 0.0F, diagonal = 0.0F;
        std::string bad;            // why the grid cannot be traced ("" = it can)
        DevBuf<float> density;
    };
    std::vector<VolGridHost> vl_grids;
    std::vector<VolMedium> vl_med_host;     // what vol_decode made of the materials, before the grids are bound
    DevBuf<atn_vg::Grid> vl_grid_desc;
    DevBuf<uint4> vl_c_smp;
    std::string vl_grid_refuse;     // why a material's grid medium cannot be rendered ("" = it can, or no material names a grid)
    bool vl_use_grid = false;       // a material names a valid grid: the frame launches the GRID flavours

    // Marks the media that name a grid (kVolGridFlag, the grid's index, the majorant in sigma_t) and uploads the medium records.
    // Runs where nothing is in flight: behind vol_decode and in volume_set_grids.
    int vol_bind_grids()
    {
        std::vector<VolMedium> med = vl_med_host;
        vl_grid_refuse.clear();
        vl_use_grid = false;
        const size_t nm = med.empty() ? 0 : med.size() - 1;
        for (size_t i = 0; i < nm && i < src.materials.size(); i++) {
            const atn_material_param& m = src.materials[i];
            if (!m.is_medium) continue;
            atn_medium_param mp;
            std::memcpy(&mp, m.medium, sizeof(mp));
            if (mp.grid_idx < 0) continue;
            const std::string who = "material " + std::to_string(i) + " is a heterogeneous medium (grid_idx " + std::to_string(mp.grid_idx) + "): ";
            std::string why;
            if ((size_t)mp.grid_idx >= vl_grids.size())
                why = "atn_volume_set_grids has set " + std::to_string(vl_grids.size()) + " grids";
            else {
                const VolGridHost& g = vl_grids[(size_t)mp.grid_idx];
                if (!g.bad.empty()) why = "its grid has " + g.bad;
                else if (mp.sigma_a != 0.0F) why = "a grid medium needs sigma_a == 0 (only scattering is tracked)";
                else if (!std::isfinite(mp.majorant) || !(mp.majorant > 0.0F)) why = "its majorant is not a finite value > 0";
                else if (mp.majorant < mp.sigma_s * g.max_density) why = "its majorant is below sigma_s * max density (a scattering probability would exceed 1)";
                else if (mp.majorant * g.diagonal > atn_vg::kVolGridStepsBound) why = "majorant * box diagonal > 1024 expected tracking steps across the grid";
            }
            if (!why.empty()) { if (vl_grid_refuse.empty()) vl_grid_refuse = who + why; continue; }
            med[i].flags |= kVolGridFlag | ((uint32_t)mp.grid_idx << kVolGridShift);
            med[i].sigma_t = mp.majorant;
            vl_use_grid = true;
        }
        if (!vl_grid_refuse.empty()) vl_use_grid = false;
        if (!med.empty()) { ATN_HIP(vl_med.upload(med, stream)); ATN_HIP(hipStreamSynchronize(stream)); }      // (`med` is pageable host memory)
        return ATN_OK;
    }

    int volume_set_grids(const atn_volume_grid* grids, uint32_t n)
    {
        if (n && !grids) return fail(ATN_ERR_INVALID_ARG, "null grid array");
        if (n > (1u << 16)) return fail(ATN_ERR_INVALID_ARG, "more than 65536 grids");
        for (uint32_t i = 0; i < n; i++) if (!grids[i].density) return fail(ATN_ERR_INVALID_ARG, "a grid without densities");
        ATN_HIP(hipSetDevice(device));
        { int q = quiesce(); if (q) return q; }
        std::vector<VolGridHost> next(n);
        std::vector<atn_vg::Grid> desc(n, atn_vg::Grid{});
        for (uint32_t i = 0; i < n; i++) {
            const atn_volume_grid& g = grids[i];
            VolGridHost& h = next[i];
            for (int k = 0; k < 3; k++) h.dim[k] = g.dim[k];
            if (g.dim[0] <= 0 || g.dim[1] <= 0 || g.dim[2] <= 0) { h.bad = "a dim component <= 0"; continue; }
            if (!std::isfinite(g.voxel_size) || !(g.voxel_size > 0.0F)) { h.bad = "a voxel_size that is not a finite value > 0"; continue; }
            const uint64_t cells = (uint64_t)g.dim[0] * (uint64_t)g.dim[1] * (uint64_t)g.dim[2];
            if (cells > (1ull << 30)) { h.bad = "more than 2^30 voxels"; continue; }
            float mx = 0.0F;
            for (uint64_t c = 0; c < cells && h.bad.empty(); c++) {
                const float d = g.density[c];
                if (!std::isfinite(d)) h.bad = "a density that is not finite";
                else if (d < 0.0F) h.bad = "a density < 0";
                else if (d > mx) mx = d;
            }
            if (!h.bad.empty()) continue;
            h.max_density = mx;
            const double ex = (double)g.dim[0] * g.voxel_size, ey = (double)g.dim[1] * g.voxel_size, ez = (double)g.dim[2] * g.voxel_size;
            h.diagonal = (float)std::sqrt(ex * ex + ey * ey + ez * ez);
            ATN_HIP(h.density.resize((size_t)cells));
            ATN_HIP(hipMemcpy(h.density.p, g.density, (size_t)cells * sizeof(float), hipMemcpyHostToDevice));
            desc[i] = atn_vg::make_grid(h.density.p, g.dim, g.origin, g.voxel_size);
        }
        vl_grids = std::move(next);
        ATN_HIP(vl_grid_desc.upload(desc, stream));
        ATN_HIP(hipStreamSynchronize(stream));
        return vol_bind_grids();
    }

    int vol_decode(const std::vector<DevMaterial>& mats)
    {
        const size_t nm = src.materials.size();
        std::vector<VolMedium> med(nm + 1, VolMedium{});       // (+ the white-diffuse fallback: no medium)
        vl_refuse.clear();
        vl_stencil = vl_carpaint = vl_toon = false;
        bool any_maybe_alpha = false;
        for (size_t i = 0; i < nm; i++) {
            const atn_material_param& m = src.materials[i];
            if (m.stencil_type == 2) vl_stencil = true;         // StencilType::STENCIL
            if (m.type == ATN_MTRL_CARPAINT) vl_carpaint = true;
            if (m.type == ATN_MTRL_TOON || m.type == ATN_MTRL_STYLIZED_BRDF) vl_toon = true;
            if (!m.is_medium) continue;
            atn_medium_param mp;
            std::memcpy(&mp, m.medium, sizeof(mp));
            VolMedium& v = med[i];
            v.g = mp.phase_function_g; v.sigma_a = mp.sigma_a; v.sigma_s = mp.sigma_s;
            v.flags = kVolMediumFlag | (m.type == ATN_MTRL_VOLUME ? kVolPureFlag : 0u);
            v.le[0] = mp.le[0]; v.le[1] = mp.le[1]; v.le[2] = mp.le[2];
            v.sigma_t = mp.sigma_a + mp.sigma_s;
            if (!vl_refuse.empty()) continue;
            if (!(mp.sigma_a + mp.sigma_s > 0.0F)) vl_refuse = "material " + std::to_string(i) + " is a medium with sigma_a + sigma_s <= 0";
            else if ((uint32_t)m.id != i) vl_refuse = "material " + std::to_string(i) + " is a medium whose id is not its index (the medium stack holds material ids)";
        }
        for (const DevMaterial& dm : mats) if (dm.attrib & kAttrMaybeAlpha) any_maybe_alpha = true;
        vl_alpha = src.config.enable_alpha_blending != 0 && any_maybe_alpha;
        vl_eps_bias = src.config.epsilon_bias_for_traversing_shadow_ray_in_medium;
        vl_med_host = std::move(med);
        return vol_bind_grids();       // (a medium with grid_idx >= 0: its grid is looked up, or the frame is refused)
    }

    int vol_ensure(int32_t w, int32_t h)
    {
        const size_t ns = n_slots;
        ATN_HIP(vl_stack.resize(ns)); ATN_HIP(vl_meta.resize(ns)); ATN_HIP(vl_hit_t.resize(ns)); ATN_HIP(vl_ev_o.resize(ns)); ATN_HIP(vl_ev_d.resize(ns));
        ATN_HIP(vl_c_o.resize(ns)); ATN_HIP(vl_c_d.resize(ns)); ATN_HIP(vl_c_w.resize(ns)); ATN_HIP(vl_c_a.resize(ns)); ATN_HIP(vl_c_b.resize(ns));
        ATN_HIP(vl_c_c.resize(ns)); ATN_HIP(vl_c_stack.resize(ns)); ATN_HIP(vl_conn_q.resize(ns)); ATN_HIP(vl_segs.resize(ns));
        ATN_HIP(vl_counters.resize(kVolCounters));
        if (!vl_grids.empty()) ATN_HIP(vl_c_smp.resize(ns));
        if (vl_capture >= 0) {
            const size_t n = (size_t)w * h;
            ATN_HIP(vl_st_state.resize(n)); ATN_HIP(vl_st_stack.resize(n)); ATN_HIP(vl_st_ray.resize(2 * n)); ATN_HIP(vl_st_conn.resize(3 * n));
        }
        vl_w = w; vl_h = h;
        return ATN_OK;
    }

    // ≙ VolumePathTracing::OnRender (volume_pathtracing.cpp:436-533) in idaten::VolumeRendering's wavefront shape: per sample, 8
    // iterations of closest hit, shade and connection walk -- a fixed number of launches, nothing is read back
    int volume_render(const atn_destination* d, atn_vec4* out_host)
    {
        { const int sr = sph_refuse("the volume renderer does not trace sphere leaves"); if (sr) return sr; }
        int rc = check_ready(d);
        if (rc) return rc;
        if (!vl_grid_refuse.empty()) return fail(ATN_ERR_UNSUPPORTED, ("volume frames: " + vl_grid_refuse).c_str());
        if (!vl_refuse.empty()) return fail(ATN_ERR_UNSUPPORTED, ("volume frames: " + vl_refuse).c_str());
        if (vl_stencil) return fail(ATN_ERR_UNSUPPORTED, "volume frames do not skip through StencilType::STENCIL materials");
        if (vl_alpha) return fail(ATN_ERR_UNSUPPORTED, "volume frames do not skip through translucent-by-alpha surfaces: alpha blending is on and a material's alpha may be < 1");
        if (vl_carpaint) return fail(ATN_ERR_UNSUPPORTED, "volume frames do not draw CarPaint's extra dimension: CarPaint materials are refused");
        if (vl_toon) return fail(ATN_ERR_UNSUPPORTED, "volume frames do not shade Toon / Stylized materials");
        if (world != 1) return fail(ATN_ERR_UNSUPPORTED, "volume frames need the whole frame on one GPU (atn_set_screen_shard world 1)");
        if (regen_mode != 0) return fail(ATN_ERR_UNSUPPORTED, "volume frames run the serial sample loop: switch path regeneration off (atn_set_regeneration(0))");
        if (shade_math_relaxed) return fail(ATN_ERR_UNSUPPORTED, "volume frames have no relaxed-math kernels: atn_set_shade_math(0)");
        if (d->count_stats) return fail(ATN_ERR_UNSUPPORTED, "volume frames do not count rays (count_stats must be 0)");
        if (d->maxDepth > 254) return fail(ATN_ERR_UNSUPPORTED, "volume frames keep depth_count in 8 bits (maxDepth <= 254)");
        ATN_HIP(hipSetDevice(device));
        rc = begin_frame(*d, frames_in_flight > 1);
        if (rc) return rc;
        rc = vol_ensure(d->width, d->height);
        if (rc) return rc;
        const bool prof = d->profile != 0;
        FrameParams fp = frame_params(*d);
        PathBuffers pb = buffers(false);
        const PassPlan plan = plan_pass(PassKind::Serial, n_slots);
        const RayLaunch vlc = ray_launch(plan, n_slots, n_slots, plan.trace_grid);
        VolArgs va{};
        va.med = vl_med.p; va.stack = vl_stack.p; va.meta = vl_meta.p; va.hit_t = vl_hit_t.p; va.ev_o = vl_ev_o.p; va.ev_d = vl_ev_d.p;
        va.c_o = vl_c_o.p; va.c_d = vl_c_d.p; va.c_w = vl_c_w.p; va.c_a = vl_c_a.p; va.c_b = vl_c_b.p; va.c_c = vl_c_c.p; va.c_stack = vl_c_stack.p;
        va.conn_q = vl_conn_q.p; va.segs = vl_segs.p; va.counters = vl_counters.p; va.eps_bias = vl_eps_bias;
        va.capture = vl_capture;
        const bool grid = vl_use_grid;      // a material names a grid: the GRID flavours of the shade kernel and the connection walk
        const VolGridArgs vg{ vl_grid_desc.p, vl_c_smp.p };
        if (vl_capture >= 0) { va.st_state = vl_st_state.p; va.st_stack = vl_st_stack.p; va.st_ray = vl_st_ray.p; va.st_conn = vl_st_conn.p; }
        // the iteration's queue counters are the volume renderer's own (9 entries: the frame's are sized by maxDepth)
        pb.q_count = vl_counters.p + kVolCntQueue;

        const uint32_t g_slots = grid_for(n_slots), g_all = (n_slots + 255u) / 256u;
        // the previous volume frame (another bank's stream) still reads and writes the per-slot state
        if (frames_in_flight > 1) ATN_HIP(vl_fence.wait(stream));
        if (vl_capture >= 0) {
            const size_t n = (size_t)d->width * d->height;
            ATN_HIP(hipMemsetAsync(vl_st_state.p, 0, n * sizeof(uint4), stream)); ATN_HIP(hipMemsetAsync(vl_st_stack.p, 0, n * sizeof(uint4), stream));
            ATN_HIP(hipMemsetAsync(vl_st_ray.p, 0, 2 * n * sizeof(float4), stream)); ATN_HIP(hipMemsetAsync(vl_st_conn.p, 0, 3 * n * sizeof(float4), stream));
        }
        ATN_HIP(hipMemsetAsync(vl_counters.p, 0, (size_t)kVolCounters * sizeof(uint32_t), stream));
        for (int32_t s = 0; s < d->sample; s++) {
            fp.sample = s;
            if (s > 0) ATN_HIP(hipMemsetAsync(vl_counters.p, 0, (size_t)kVolCntFrame * sizeof(uint32_t), stream));
            prof_begin(prof, ATN_K_GEN);
            hipLaunchKernelGGL(k_gen_path, dim3(g_slots), dim3(256), 0, stream, pb, fp, camera, (const uint32_t*)seeds.p);
            vol_launch_begin(vlc, stream, fp, va);
            prof_end(prof);
            for (int32_t it = 0; it < kVolIterations; it++) {
                prof_begin(prof, ATN_K_TRACE_CLOSEST);
                vol_launch_closest(vlc, stream, pb, scene, va, it);
                prof_end(prof);
                prof_begin(prof, ATN_K_SHADE);
                if (grid) vol_launch_shade_grid(scene.material_set, vlc, stream, pb, scene, fp, camera, va, vg, it);
                else vol_launch_shade(scene.material_set, vlc, stream, pb, scene, fp, camera, va, it);
                prof_end(prof);
                prof_begin(prof, ATN_K_TRACE_FUSED);
                if (grid) vol_launch_transmit_grid(vlc, stream, pb, scene, va, vg, it);
                else vol_launch_transmit(vlc, stream, pb, scene, va, it);
                prof_end(prof);
            }
            if (d->sample > 1) {
                prof_begin(prof, ATN_K_ACCUM);
                hipLaunchKernelGGL(k_accumulate_sample, dim3(g_all), dim3(256), 0, stream, pb, fp);
                prof_end(prof);
            }
        }
        vol_launch_reduce(vlc, stream, fp, va);
        ATN_HIP(vl_fence.record(stream));
        vl_captured = vl_capture;
        vl_rendered = true;
        rc = gather_film(*d, pb, fp);
        return rc ? rc : end_film_frame(*d, out_host);
    }

    int volume_reset()
    {
        ATN_HIP(hipSetDevice(device));
        { int q = quiesce(); if (q) return q; }
        vl_captured = -1; vl_rendered = false;
        return reset();
    }

    int volume_download(int32_t which, void* out)
    {
        if (!out) return fail(ATN_ERR_INVALID_ARG, "null output");
        if (!vl_rendered) return fail(ATN_ERR_INVALID_ARG, "no volume frame has been rendered");
        if (which != 4 && which != 5 && vl_captured < 0) return fail(ATN_ERR_INVALID_ARG, "the last volume frame kept no stage buffers: atn_volume_capture(ctx, iteration) before the frame");
        const size_t n = (size_t)vl_w * vl_h;
        const StageBuf bufs[] = { { vl_st_state.p, n * sizeof(uint4) }, { vl_st_stack.p, n * sizeof(uint4) }, { vl_st_ray.p, 2 * n * sizeof(float4) },
                                  { vl_st_conn.p, 3 * n * sizeof(float4) }, { vl_counters.p + kVolCntFrame, 4 * sizeof(uint32_t) },
                                  { vl_counters.p + kVolCntFrame + 4, 2 * sizeof(uint32_t) } };
        return download_stage(bufs, which, out, "no such volume buffer");
    }

    int volume_phase_table(float g, uint32_t n, const float* w, const float* r1, const float* r2, const float* wo, float* out_dir, float* out_eval)
    {
        if (!n || !w || !r1 || !r2 || !wo || !out_dir || !out_eval) return fail(ATN_ERR_INVALID_ARG, "null argument / no cases");
        ATN_HIP(hipSetDevice(device));
        DevBuf<float> dw, d1, d2, dwo, dd, de;
        ATN_HIP(dw.resize(3 * (size_t)n)); ATN_HIP(d1.resize(n)); ATN_HIP(d2.resize(n)); ATN_HIP(dwo.resize(3 * (size_t)n));
        ATN_HIP(dd.resize(3 * (size_t)n)); ATN_HIP(de.resize(n));
        ATN_HIP(hipMemcpyAsync(dw.p, w, 12 * (size_t)n, hipMemcpyHostToDevice, stream));
        ATN_HIP(hipMemcpyAsync(d1.p, r1, 4 * (size_t)n, hipMemcpyHostToDevice, stream));
        ATN_HIP(hipMemcpyAsync(d2.p, r2, 4 * (size_t)n, hipMemcpyHostToDevice, stream));
        ATN_HIP(hipMemcpyAsync(dwo.p, wo, 12 * (size_t)n, hipMemcpyHostToDevice, stream));
        vol_launch_phase_table(stream, g, n, dw.p, d1.p, d2.p, dwo.p, dd.p, de.p);
        ATN_HIP(hipGetLastError());
        ATN_HIP(hipMemcpyAsync(out_dir, dd.p, 12 * (size_t)n, hipMemcpyDeviceToHost, stream));
        ATN_HIP(hipMemcpyAsync(out_eval, de.p, 4 * (size_t)n, hipMemcpyDeviceToHost, stream));
        ATN_HIP(hipStreamSynchronize(stream));
        return ATN_OK;
    }

    // ------------------------------------------------------------------------------------------------
    // Ambient occlusion (aten::AORenderer / idaten::AORenderer, device/ao.hpp; docs/AO.md): the ray list, the per-slot and per-pixel
    // planes.  The state is shared by the banks: an event orders consecutive AO frames.
    // ------------------------------------------------------------------------------------------------
    AoRayList ao_list;
    DevBuf<float4> ao_st_ray, ao_st_ans;
    DevBuf<float> ao_depth_s, ao_value, ao_depth;
    int32_t ao_num_rays = 1, ao_filter = 0;     // AORenderer's member defaults (aorenderer.h) and its active branch
    float ao_radius = 1.0F;
    int32_t ao_w = 0, ao_h = 0, ao_capture = 0;
    bool ao_captured = false, ao_rendered = false;
    FrameFence ao_fence;        // the last AO frame's kernels are done with the AO state (the next frame waits for it)

    int ao_set_params(int32_t num_rays, float radius, int32_t filter)
    {
        if (num_rays < 1 || num_rays > kAoMaxRays) return fail(ATN_ERR_INVALID_ARG, "AO: num_rays must be 1..64");
        if (!(radius > 0.0F) || !std::isfinite(radius)) return fail(ATN_ERR_INVALID_ARG, "AO: the radius must be positive and finite");
        if (filter != 0 && filter != 1) return fail(ATN_ERR_INVALID_ARG, "AO: filter is 0 or 1");
        ao_num_rays = num_rays; ao_radius = radius; ao_filter = filter;
        return ATN_OK;
    }

    // the planes start at zero (path_host_'s contributions, the film) and persist across frames
    int ao_ensure(int32_t w, int32_t h)
    {
        const size_t r = (size_t)ao_num_rays * n_slots;
        if (r > (size_t)kAoRayMask) return fail(ATN_ERR_UNSUPPORTED, "AO frames list at most 2^28 rays (fewer rays per pixel, or a smaller frame)");
        ATN_HIP(ao_list.ensure(r, n_slots, w, h));
        ATN_HIP(ao_depth_s.resize(n_slots));
        const size_t n = (size_t)w * h;
        if (w != ao_w || h != ao_h) {
            ATN_HIP(ao_value.resize(n)); ATN_HIP(ao_depth.resize(n));
            ATN_HIP(hipMemsetAsync(ao_list.state.p, 0, n * sizeof(uint32_t), stream));
            ATN_HIP(hipMemsetAsync(ao_value.p, 0, n * sizeof(float), stream));
            ATN_HIP(hipMemsetAsync(ao_depth.p, 0, n * sizeof(float), stream));
            ao_w = w; ao_h = h;
        }
        if (ao_capture) { ATN_HIP(ao_st_ray.resize(2 * n)); ATN_HIP(ao_st_ans.resize(n)); }
        return ATN_OK;
    }

    // ≙ AORenderer::RenderAO / RenderAOWithBilateralFilter (aorenderer.cpp:71-275) in idaten::AORenderer's wavefront shape: a fixed
    // number of launches, nothing is read back
    int ao_render(const atn_destination* dst, atn_vec4* out_host)
    {
        { const int sr = sph_refuse("the AO renderer does not trace sphere leaves"); if (sr) return sr; }
        if (!dst) return fail(ATN_ERR_INVALID_ARG, "null destination");
        atn_destination d1 = *dst;      // the reference reads neither sample nor maxDepth
        d1.maxDepth = 1; d1.russianRouletteDepth = 1; d1.sample = 1;
        const atn_destination* d = &d1;
        int rc = check_ready(d);
        if (rc) return rc;
        if (np_carpaint) return fail(ATN_ERR_UNSUPPORTED, "AO frames do not draw applyNormal's CarPaint flake samples: CarPaint materials are refused");
        if (world != 1) return fail(ATN_ERR_UNSUPPORTED, "AO frames need the whole frame on one GPU (atn_set_screen_shard world 1)");
        if (regen_mode != 0) return fail(ATN_ERR_UNSUPPORTED, "AO frames have one sample per pixel: switch path regeneration off (atn_set_regeneration(0))");
        if (shade_math_relaxed) return fail(ATN_ERR_UNSUPPORTED, "AO frames have no relaxed-math kernels: atn_set_shade_math(0)");
        if (d->count_stats) return fail(ATN_ERR_UNSUPPORTED, "AO frames do not count rays (count_stats must be 0)");
        if (ao_filter && d->break_on_terminate) return fail(ATN_ERR_UNSUPPORTED, "AO: the bilateral filter over rows the CPU renderer leaves unwritten would filter earlier frames' planes: filter = 1 needs break_on_terminate = 0");
        ATN_HIP(hipSetDevice(device));
        if (frames_in_flight > 1 && (d->width != ao_w || d->height != ao_h || ao_list.would_grow((size_t)ao_num_rays * n_slots, n_slots, d->width, d->height) || (ao_capture && !ao_st_ans.p))) { rc = quiesce(); if (rc) return rc; }
        rc = begin_frame(*d, frames_in_flight > 1);
        if (rc) return rc;
        if (frames_in_flight > 1 && ao_list.would_grow((size_t)ao_num_rays * n_slots, n_slots, d->width, d->height)) { rc = quiesce(); if (rc) return rc; }
        rc = ao_ensure(d->width, d->height);
        if (rc) return rc;
        const bool prof = d->profile != 0;
        auto [fp, pb, plan] = serial_frame(*d);
        AoArgs aa = ao_list.args();
        aa.depth_s = ao_depth_s.p; aa.value = ao_value.p; aa.depth = ao_depth.p;
        aa.num_rays = ao_num_rays; aa.radius = ao_radius; aa.literal = d->break_on_terminate ? 1 : 0; aa.filter = ao_filter;
        if (ao_capture) { aa.st_ray = ao_st_ray.p; aa.st_ans = ao_st_ans.p; }
        // the walk of the AO rays: the frame's walk, LDS copy and block, num_rays rays per path
        const uint32_t n_rays = (uint32_t)ao_num_rays * n_slots;
        const RayLaunch al = ray_launch(plan, n_slots, n_rays, trace_grid(n_rays, true));

        // the previous AO frame (another bank's stream) still reads and writes the AO state
        if (frames_in_flight > 1) ATN_HIP(ao_fence.wait(stream));
        if (ao_capture) {
            const size_t n = (size_t)d->width * d->height;
            ATN_HIP(hipMemsetAsync(ao_st_ray.p, 0, 2 * n * sizeof(float4), stream));
            ATN_HIP(hipMemsetAsync(ao_st_ans.p, 0, n * sizeof(float4), stream));
        }
        ATN_HIP(hipMemsetAsync(counters.p, 0, (size_t)4 * counters_depth * 4, stream));
        ATN_HIP(hipMemsetAsync(ao_list.counters.p, 0, (size_t)kAoCounters * sizeof(uint32_t), stream));
        ATN_HIP(hipMemsetAsync(ao_list.row_min.p, 0xff, (size_t)d->height * sizeof(uint32_t), stream));
        prof_begin(prof, ATN_K_GEN);
        hipLaunchKernelGGL(k_gen_path, dim3(grid_for(n_slots)), dim3(256), 0, stream, pb, fp, camera, (const uint32_t*)seeds.p);
        prof_end(prof);
        prof_begin(prof, ATN_K_TRACE_CLOSEST);
        ao_launch_primary(trace_launch(plan, 0), stream, pb, scene, aa);
        prof_end(prof);
        prof_begin(prof, ATN_K_SHADE);
        ao_launch_rays(al, stream, pb, scene, fp, aa);
        prof_end(prof);
        rc = wait_film();
        if (rc) return rc;
        prof_begin(prof, ATN_K_GATHER);
        ao_launch_resolve(al, stream, fp, aa, film.p, tile_out.p);
        prof_end(prof);
        ATN_HIP(hipGetLastError());
        ATN_HIP(ao_fence.record(stream));
        ao_captured = ao_capture != 0;
        ao_rendered = true;
        return end_film_frame(*d, out_host);
    }

    // the film and the AO planes of a fresh context
    int ao_reset()
    {
        ATN_HIP(hipSetDevice(device));
        { int q = quiesce(); if (q) return q; }
        if (ao_list.state.p) {
            const size_t n = (size_t)ao_w * ao_h;
            ATN_HIP(hipMemsetAsync(ao_list.state.p, 0, n * sizeof(uint32_t), stream));
            ATN_HIP(hipMemsetAsync(ao_value.p, 0, n * sizeof(float), stream));
            ATN_HIP(hipMemsetAsync(ao_depth.p, 0, n * sizeof(float), stream));
        }
        ao_captured = false; ao_rendered = false;
        return reset();
    }

    int ao_download(int32_t which, void* out)
    {
        if (!out) return fail(ATN_ERR_INVALID_ARG, "null output");
        if (!ao_rendered) return fail(ATN_ERR_INVALID_ARG, "no AO frame has been rendered");
        if (which >= 4 && !ao_captured) return fail(ATN_ERR_INVALID_ARG, "the last AO frame kept no stage buffers: atn_ao_capture(ctx, 1) before the frame");
        const size_t n = (size_t)ao_w * ao_h;
        const StageBuf bufs[] = { { ao_list.state.p, n * sizeof(uint32_t) }, { ao_value.p, n * sizeof(float) }, { ao_depth.p, n * sizeof(float) },
                                  { ao_list.row_min.p, (size_t)ao_h * sizeof(uint32_t) }, { ao_st_ray.p, 2 * n * sizeof(float4) }, { ao_st_ans.p, n * sizeof(float4) } };
        return download_stage(bufs, which, out, "no such AO buffer");
    }

    // ------------------------------------------------------------------------------------------------
    // The NPR shadow pre-pass (aten::NprPathTracer::OnRender's first pass / idaten's onShadeByShadowRay, device/npr_shadow.hpp;
    // docs/NPR_SHADOW.md).  The planes belong to the BANK (they rotate with it, swap_bank): a frame in flight keeps its own plane, so
    // the next frame's pre-pass -- on another bank's stream -- overwrites nothing this frame's shade launches still read, and nothing
    // orders the two.
    // ------------------------------------------------------------------------------------------------
    DevBuf<float> ns_f_lit, ns_f_depth, ns_f_out;               // atn_npr_shadow_filter's own
    // the planes of the last frame that ran the pre-pass, whichever bank is current now (atn_npr_shadow_download): they stay valid until
    // that bank runs its next pre-pass, which becomes the last one
    const float* ns_last[3] = {};
    int32_t ns_last_w = 0, ns_last_h = 0;
    int32_t ns_mode = 0;            // atn_npr_shadow_set_mode
    bool ns_any = false;            // an uploaded Toon / StylizedBrdf material has stylized_shadow.enable (upload)
    bool ns_rendered = false;

    // NPR hatching (idaten::NPRPathTracing's HatchingShadowBase x HatchingShadowDirection; device/npr_hatching.hpp,
    // docs/NPR_HATCHING.md): what mode 1's pre-pass filters (0 the AO value at the primary hit, 1 the bounce-0 lit bit) and how (0 None,
    // 1 Horizontal, 2 Vertical, 3 Orthogonal, 4 Cross, 5 OrthogonalCross).  The defaults are the pre-pass as it was, launch for launch.
    int32_t nh_base = 1, nh_dir = kHatchHorizontal, nh_num_rays = 1;
    float nh_radius = 1.0F;
    int32_t ns_last_base = 1;               // the base of the last frame that ran the pre-pass
    const float* nh_last_first = nullptr;   // its first step's plane (the final plane of a one-step direction)
    DevBuf<float> nh_f_first;               // atn_npr_hatching_filter's own

    int nh_set(int32_t base, int32_t direction, int32_t num_rays, float radius)
    {
        if (base != 0 && base != 1) return fail(ATN_ERR_INVALID_ARG, "NPR hatching: base is 0 (AO) or 1 (the shadow ray)");
        if (direction < kHatchNone || direction > kHatchOrthogonalCross) return fail(ATN_ERR_INVALID_ARG, "NPR hatching: direction is 0 None, 1 Horizontal, 2 Vertical, 3 Orthogonal, 4 Cross or 5 OrthogonalCross");
        if (num_rays < 1 || num_rays > kAoMaxRays) return fail(ATN_ERR_INVALID_ARG, "NPR hatching: ao_num_rays must be 1..64");
        if (!(radius > 0.0F) || !std::isfinite(radius)) return fail(ATN_ERR_INVALID_ARG, "NPR hatching: ao_radius must be positive and finite");
        nh_base = base; nh_dir = direction; nh_num_rays = num_rays; nh_radius = radius;
        return ATN_OK;
    }

    // what the AO base cannot do on top of mode 1's refusals (atn_render and atn_npr_render, in front of the frame)
    int nh_check(const atn_destination* d)
    {
        if (ns_mode != 1 || nh_base != 0) return ATN_OK;
        if ((uint64_t)nh_num_rays * (uint64_t)d->width * (uint64_t)d->height > (uint64_t)kAoRayMask)
            return fail(ATN_ERR_UNSUPPORTED, "NPR hatching: the AO base lists at most 2^28 rays per frame (fewer rays per pixel, or a smaller frame)");
        return ATN_OK;
    }

    // would nh_ensure replace a buffer of this bank?  (with frames in flight the caller waits for them first)
    bool nh_grows(int32_t w, int32_t h) const
    {
        const size_t n = (size_t)w * h;
        if (nh_dir >= kHatchCross && n > nh_first.n) return true;
        if (nh_base != 0) return false;
        return nh_list.would_grow((size_t)nh_num_rays * n_slots, n_slots, w, h);
    }

    int nh_ensure(int32_t w, int32_t h)
    {
        const size_t n = (size_t)w * h;
        if (nh_dir >= kHatchCross) ATN_HIP(nh_first.resize(n));
        if (nh_base != 0) return ATN_OK;
        const size_t r = (size_t)nh_num_rays * n_slots;
        if (r > (size_t)kAoRayMask) return fail(ATN_ERR_UNSUPPORTED, "NPR hatching: the AO base lists at most 2^28 rays per frame (fewer rays per pixel, or a smaller frame)");
        ATN_HIP(nh_list.ensure(r, n_slots, w, h));
        return ATN_OK;
    }

    int ns_set_mode(int32_t mode)
    {
        if (mode != 0 && mode != 1) return fail(ATN_ERR_INVALID_ARG, "NPR shadow: mode is 0 (the uploaded texture) or 1 (the shadow-ray pre-pass)");
        ns_mode = mode;
        return ATN_OK;
    }

    // does this frame run the pre-pass?
    bool ns_frame() const { return ns_mode == 1 && ns_any; }

    // what mode 1 cannot do in atn_render (atn_npr_render refuses the same configurations itself, mode 1 or not)
    int ns_check(const atn_destination* d)
    {
        if (ns_mode != 1) return ATN_OK;
        if (world != 1) return fail(ATN_ERR_UNSUPPORTED, "NPR shadow pre-pass: the row filter crosses tiles, the whole frame has to be on one GPU (atn_set_screen_shard world 1)");
        if (regen_mode != 0) return fail(ATN_ERR_UNSUPPORTED, "NPR shadow pre-pass: frames run the serial sample loop: switch path regeneration off (atn_set_regeneration(0))");
        if (shade_math_relaxed) return fail(ATN_ERR_UNSUPPORTED, "NPR shadow pre-pass: there are no relaxed-math kernels: atn_set_shade_math(0)");
        if (d->count_stats) return fail(ATN_ERR_UNSUPPORTED, "NPR shadow pre-pass: its rays are not counted (count_stats must be 0)");
        if (np_carpaint) return fail(ATN_ERR_UNSUPPORTED, "NPR shadow pre-pass: applyNormal's CarPaint flake samples are not drawn: CarPaint materials are refused");
        return nh_check(d);
    }

    int ns_ensure(int32_t w, int32_t h)
    {
        if (n_slots != ns_slots) { ATN_HIP(ns_depth_s.resize(n_slots)); ns_slots = n_slots; }
        if (w != ns_w || h != ns_h) {
            const size_t n = (size_t)w * h;
            ATN_HIP(ns_lit.resize(n)); ATN_HIP(ns_depth.resize(n)); ATN_HIP(ns_plane.resize(n));
            ns_w = w; ns_h = h;
        }
        return ATN_OK;
    }

    // The pre-pass of a frame, on the frame's stream and bank, in front of its sample loop (begin_frame has run): sample 0's paths, their
    // closest hits, the bounce-0 shadow rays, the row filter.  Leaves `scene` pointing at the plane: ns_end_frame() puts the uploaded
    // texture back once the frame's launches are enqueued (kernel arguments are copied at the launch).
    const float* ns_saved_tex = nullptr;
    int32_t ns_saved_w = 0, ns_saved_h = 0;
    bool ns_swapped = false;
    int ns_prepass(const atn_destination* d)
    {
        if (frames_in_flight > 1 && (d->width != ns_w || d->height != ns_h || n_slots != ns_slots || nh_grows(d->width, d->height))) { const int q = quiesce(); if (q) return q; }
        int rc = ns_ensure(d->width, d->height);
        if (rc) return rc;
        rc = nh_ensure(d->width, d->height);
        if (rc) return rc;
        const bool prof = d->profile != 0;
        auto [fp, pb, plan] = serial_frame(*d);
        ATN_HIP(hipMemsetAsync(counters.p, 0, (size_t)4 * counters_depth * 4, stream));
        prof_begin(prof, ATN_K_GEN);
        hipLaunchKernelGGL(k_gen_path, dim3(grid_for(n_slots)), dim3(256), 0, stream, pb, fp, camera, (const uint32_t*)seeds.p);
        prof_end(prof);
        if (nh_base != 0) {
            NsArgs na{};
            na.depth_s = ns_depth_s.p; na.lit = ns_lit.p; na.depth = ns_depth.p; na.plane = ns_plane.p;
            prof_begin(prof, ATN_K_TRACE_CLOSEST);
            ns_launch_primary(trace_launch(plan, 0), stream, pb, scene, na);
            prof_end(prof);
            prof_begin(prof, ATN_K_SHADE);
            ns_launch_rays(ray_launch(plan, n_slots, n_slots, trace_grid(n_slots, true)), stream, pb, scene, fp, na);
        }
        else {
            // the AO base: ShandeByAO at every primary hit through the AO renderer's own kernels and sampler (docs/NPR_HATCHING.md), over
            // this bank's ray list; the source plane (ns_lit) then holds AO values, and there is no lit bit
            AoArgs aa = nh_list.args();
            aa.depth_s = ns_depth_s.p; aa.value = ns_lit.p; aa.depth = ns_depth.p;
            aa.num_rays = nh_num_rays; aa.radius = nh_radius;
            const uint32_t n_rays = (uint32_t)nh_num_rays * n_slots;
            const RayLaunch al = ray_launch(plan, n_slots, n_rays, trace_grid(n_rays, true));
            ATN_HIP(hipMemsetAsync(nh_list.counters.p, 0, (size_t)kAoCounters * sizeof(uint32_t), stream));
            ATN_HIP(hipMemsetAsync(nh_list.row_min.p, 0xff, (size_t)d->height * sizeof(uint32_t), stream));
            prof_begin(prof, ATN_K_TRACE_CLOSEST);
            ao_launch_primary(trace_launch(plan, 0), stream, pb, scene, aa);
            prof_end(prof);
            prof_begin(prof, ATN_K_SHADE);
            ao_launch_rays(al, stream, pb, scene, fp, aa);
            nh_launch_resolve(al.slot_grid, stream, fp, aa, ns_lit.p, ns_depth.p);
        }
        const bool two_step = nh_dir >= kHatchCross;
        if (nh_dir == kHatchHorizontal) ns_launch_filter(stream, ns_lit.p, ns_depth.p, ns_plane.p, d->width, d->height);
        else nh_launch_filter(nh_dir, stream, ns_lit.p, ns_depth.p, two_step ? nh_first.p : nullptr, ns_plane.p, d->width, d->height);
        prof_end(prof);
        ATN_HIP(hipGetLastError());
        ns_saved_tex = scene.screen_shadow; ns_saved_w = scene.ss_w; ns_saved_h = scene.ss_h;
        scene.screen_shadow = ns_plane.p; scene.ss_w = d->width; scene.ss_h = d->height;
        ns_swapped = true;
        ns_rendered = true;
        ns_last[0] = ns_plane.p; ns_last[1] = ns_lit.p; ns_last[2] = ns_depth.p;
        ns_last_base = nh_base; nh_last_first = two_step ? nh_first.p : ns_plane.p;
        ns_last_w = d->width; ns_last_h = d->height;
        return ATN_OK;
    }
    // behind the frame's last shade launch (on `stream`, the batches joined): the uploaded texture is the scene's again
    int ns_end_frame()
    {
        if (!ns_swapped) return ATN_OK;
        scene.screen_shadow = ns_saved_tex; scene.ss_w = ns_saved_w; scene.ss_h = ns_saved_h;
        ns_swapped = false;
        return ATN_OK;
    }

    int ns_download(int32_t which, float* out, uint32_t n)
    {
        if (!out) return fail(ATN_ERR_INVALID_ARG, "null output");
        if (!ns_rendered) return fail(ATN_ERR_INVALID_ARG, "no frame has run the NPR shadow pre-pass");
        if (which < 0 || which > 2) return fail(ATN_ERR_INVALID_ARG, "no such NPR shadow plane");
        if (which == 1 && ns_last_base == 0) return fail(ATN_ERR_INVALID_ARG, "the last pre-pass filtered AO values (atn_npr_hatching_set base 0): there is no lit bit; atn_npr_hatching_download(0) has the source plane");
        if ((size_t)n != (size_t)ns_last_w * ns_last_h) return fail(ATN_ERR_INVALID_ARG, "NPR shadow planes have width x height floats");
        { const int s = settle(); if (s) return s; }
        ATN_HIP(hipMemcpy(out, ns_last[which], (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
        return ATN_OK;
    }

    // the two filter stage entries behind their argument checks: the planes up, one launch (direction < 0: the pre-pass's own row filter,
    // else the hatching filter of that direction), the result down
    int filter_planes(const float* src, const float* depth, int32_t w, int32_t h, int32_t direction, float* out)
    {
        ATN_HIP(hipSetDevice(device));
        { int q = quiesce(); if (q) return q; }
        const size_t n = (size_t)w * h;
        ATN_HIP(ns_f_lit.resize(n)); ATN_HIP(ns_f_depth.resize(n)); ATN_HIP(ns_f_out.resize(n));
        if (direction >= 0) ATN_HIP(nh_f_first.resize(n));
        ATN_HIP(hipMemcpyAsync(ns_f_lit.p, src, n * sizeof(float), hipMemcpyHostToDevice, stream));
        ATN_HIP(hipMemcpyAsync(ns_f_depth.p, depth, n * sizeof(float), hipMemcpyHostToDevice, stream));
        if (direction < 0) ns_launch_filter(stream, ns_f_lit.p, ns_f_depth.p, ns_f_out.p, w, h);
        else nh_launch_filter(direction, stream, ns_f_lit.p, ns_f_depth.p, nh_f_first.p, ns_f_out.p, w, h);
        ATN_HIP(hipGetLastError());
        ATN_HIP(hipMemcpyAsync(out, ns_f_out.p, n * sizeof(float), hipMemcpyDeviceToHost, stream));
        ATN_HIP(hipStreamSynchronize(stream));
        return ATN_OK;
    }

    // the row filter alone over uploaded planes (a stage entry for tests)
    int ns_filter(const float* lit, const float* depth, int32_t w, int32_t h, float* out)
    {
        if (!lit || !depth || !out) return fail(ATN_ERR_INVALID_ARG, "null plane");
        if (w < 1 || h < 1 || w > 16384 || h > 16384) return fail(ATN_ERR_INVALID_ARG, "NPR shadow filter: sizes are 1..16384 per side");
        return filter_planes(lit, depth, w, h, -1, out);
    }

    // 0 the unfiltered source plane of the last pre-pass (AO values / the bit as 0.0 / 1.0), 1 its first step's plane
    int nh_download(int32_t which, float* out, uint32_t n)
    {
        if (!out) return fail(ATN_ERR_INVALID_ARG, "null output");
        if (!ns_rendered) return fail(ATN_ERR_INVALID_ARG, "no frame has run the NPR shadow pre-pass");
        if (which != 0 && which != 1) return fail(ATN_ERR_INVALID_ARG, "no such NPR hatching plane");
        if ((size_t)n != (size_t)ns_last_w * ns_last_h) return fail(ATN_ERR_INVALID_ARG, "NPR hatching planes have width x height floats");
        { const int s = settle(); if (s) return s; }
        ATN_HIP(hipMemcpy(out, which == 0 ? ns_last[1] : nh_last_first, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
        return ATN_OK;
    }

    // the filter of one direction alone over uploaded planes (a stage entry for tests)
    int nh_filter(const float* src, const float* depth, int32_t w, int32_t h, int32_t direction, float* out)
    {
        if (!src || !depth || !out) return fail(ATN_ERR_INVALID_ARG, "null plane");
        if (w < 1 || h < 1 || w > 16384 || h > 16384) return fail(ATN_ERR_INVALID_ARG, "NPR hatching filter: sizes are 1..16384 per side");
        if (direction < kHatchNone || direction > kHatchOrthogonalCross) return fail(ATN_ERR_INVALID_ARG, "NPR hatching filter: direction is 0..5");
        return filter_planes(src, depth, w, h, direction, out);
    }

    // ≙ idaten::Renderer::reset, renderer.h:40-43
    // {shadow rays cast, rays that reached the light} of the deferred frames since the last reset
    int nee_deferral_stats(uint64_t out[2])
    {
        out[0] = out[1] = 0;
        if (!nee_stats.p) return ATN_OK;
        ATN_HIP(hipSetDevice(device));
        { int q = quiesce(); if (q) return q; }
        unsigned long long h[2] = {};
        ATN_HIP(hipMemcpyAsync(h, nee_stats.p, 16, hipMemcpyDeviceToHost, stream));
        ATN_HIP(hipStreamSynchronize(stream));
        out[0] = h[0]; out[1] = h[1];
        return ATN_OK;
    }

    int reset()
    {
        if (nee_stats.p) {
            ATN_HIP(hipSetDevice(device));
            { int q = quiesce(); if (q) return q; }
            ATN_HIP(hipMemsetAsync(nee_stats.p, 0, 16, stream));
        }
        if (film.p) {
            ATN_HIP(hipSetDevice(device));
            { int q = quiesce(); if (q) return q; }
            ATN_HIP(hipMemsetAsync(film.p, 0, film.n * sizeof(float4), stream));
            return record_film_writer();        // the next frame's k_gather goes behind the clear
        }
        return ATN_OK;
    }
};

} // namespace atn

#include "host/mgpu.hpp"

struct atn_ctx { atn::PathTracing r; };
struct atn_mgpu { atn::MultiGpu m; };

using atn::PathTracing;

#define CTX_OR_FAIL(ctx) do { if (!(ctx)) return ATN_ERR_INVALID_ARG; } while (0)
// every entry point except atn_render first lets the frames in flight finish (atn_set_frames_in_flight)
#define CTX_QUIET_OR_FAIL(ctx) do { if (!(ctx)) return ATN_ERR_INVALID_ARG; \
    if ((ctx)->r.frames_in_flight > 1) { int q_ = (ctx)->r.quiesce(); if (q_) return q_; } } while (0)

// No exception may cross the C boundary (std::vector growth in the upload paths can throw std::bad_alloc).
template <class F>
static int guarded(atn_ctx* ctx, F&& f) noexcept
{
    try { return f(); }
    catch (const std::bad_alloc&) {
        try { return ctx->r.fail(ATN_ERR_OUT_OF_MEMORY, "out of host memory"); } catch (...) { return ATN_ERR_OUT_OF_MEMORY; }
    }
    catch (const std::exception& e) {
        try { return ctx->r.fail(ATN_ERR_INVALID_ARG, std::string("unexpected exception: ") + e.what()); } catch (...) { return ATN_ERR_INVALID_ARG; }
    }
    catch (...) { return ATN_ERR_INVALID_ARG; }
}
#define C_HIP(r, expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return (r).fail(ATN_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); } while (0)

#define MG_OR_FAIL(mg) do { if (!(mg)) return ATN_ERR_INVALID_ARG; } while (0)
template <class F>
static int mg_guarded(atn_mgpu* mg, F&& f) noexcept
{
    try { return f(); }
    catch (const std::bad_alloc&) { try { return mg->m.fail(ATN_ERR_OUT_OF_MEMORY, "out of host memory"); } catch (...) { return ATN_ERR_OUT_OF_MEMORY; } }
    catch (...) { return ATN_ERR_INVALID_ARG; }
}

extern "C" {

int atn_create(atn_ctx** out, int device_ordinal)
{
    if (!out) return ATN_ERR_INVALID_ARG;
    *out = nullptr;
    atn_ctx* c = new (std::nothrow) atn_ctx();
    if (!c) return ATN_ERR_OUT_OF_MEMORY;
    int rc = c->r.init(device_ordinal);
    if (rc != ATN_OK) {
        std::fprintf(stderr, "atn_create: %s\n", c->r.last_error.c_str());
        delete c;
        return rc;
    }
    *out = c;
    return ATN_OK;
}

void atn_destroy(atn_ctx* ctx) { delete ctx; }

const char* atn_last_error(atn_ctx* ctx) { return ctx ? ctx->r.last_error.c_str() : "null context"; }

int atn_upload_scene(atn_ctx* ctx, const atn_scene_desc* scene)
{
    CTX_QUIET_OR_FAIL(ctx);
    if (!scene) return ctx->r.fail(ATN_ERR_INVALID_ARG, "null scene");
    return guarded(ctx, [&] { return ctx->r.UpdateSceneData(scene); });
}

int atn_set_upload_options(atn_ctx* ctx, int32_t anyhit_twin, int32_t anyhit_twin_dirs, int32_t node_layout, int32_t planar_lights)
{
    CTX_QUIET_OR_FAIL(ctx);
    if (anyhit_twin > 2 || (anyhit_twin_dirs >= 0 && anyhit_twin_dirs != 1 && anyhit_twin_dirs != 8)) return ctx->r.fail(ATN_ERR_INVALID_ARG, "upload option out of range");
    if (anyhit_twin >= 0) ctx->r.env_anyhit_twin = anyhit_twin;
    if (anyhit_twin_dirs >= 0) ctx->r.env_anyhit_twin_dirs = anyhit_twin_dirs;
    if (node_layout >= 0) ctx->r.opt_node_layout = node_layout != 0;
    if (planar_lights >= 0) ctx->r.opt_planar_lights = planar_lights != 0;
    return ATN_OK;
}
int atn_set_sphere_intersection(atn_ctx* ctx, int32_t mode)
{
    CTX_QUIET_OR_FAIL(ctx);
    if (mode < 0 || mode > 1) return ctx->r.fail(ATN_ERR_INVALID_ARG, "sphere intersection mode out of range");
    ctx->r.sphere_mode = mode;
    return ATN_OK;
}
int atn_sphere_leaves(atn_ctx* ctx, uint32_t* n)
{
    CTX_OR_FAIL(ctx);
    if (!n) return ctx->r.fail(ATN_ERR_INVALID_ARG, "null output");
    *n = ctx->r.has_scene ? ctx->r.n_sphere_leaves : 0u;
    return ATN_OK;
}
int atn_update_camera(atn_ctx* ctx, const atn_camera_param* camera) { CTX_OR_FAIL(ctx); return guarded(ctx, [&] { return ctx->r.updateCamera(camera); }); }

int atn_update_tlas(atn_ctx* ctx, const atn_object_param* objects, uint32_t n_objects, const atn_mat4* matrices, uint32_t n_matrices,
                    const atn_bvh_node* top_nodes, uint32_t n_top_nodes)
{
    CTX_OR_FAIL(ctx);      // enqueued behind the frames in flight (begin_scene_update), no host stop
    return guarded(ctx, [&] { return ctx->r.updateBVH(objects, n_objects, matrices, n_matrices, top_nodes, n_top_nodes); });
}
int atn_update_geometry(atn_ctx* ctx, const atn_vec4* vtx_pos, const atn_vec4* vtx_nml, uint32_t n_vertices, uint32_t vtx_offset,
                        const atn_triangle_param* triangles, uint32_t n_triangles, uint32_t tri_offset)
{
    CTX_OR_FAIL(ctx);
    return guarded(ctx, [&] { return ctx->r.updateGeometry(vtx_pos, vtx_nml, n_vertices, vtx_offset, triangles, n_triangles, tri_offset); });
}
// scene edits: synchronous (they wait for the frames in flight), atomic, nothing is reset
int atn_update_materials(atn_ctx* ctx, const atn_material_param* materials, uint32_t n, uint32_t first)
{
    CTX_OR_FAIL(ctx);
    return guarded(ctx, [&] { return ctx->r.update_materials(materials, n, first); });
}
int atn_update_lights(atn_ctx* ctx, const atn_light_param* lights, uint32_t n, uint32_t first, int32_t npr_target)
{
    CTX_OR_FAIL(ctx);
    return guarded(ctx, [&] { return ctx->r.update_lights(lights, n, first, npr_target); });
}
int atn_update_texture(atn_ctx* ctx, int32_t texid, const atn_texture_desc* tex)
{
    CTX_OR_FAIL(ctx);
    return guarded(ctx, [&] { return ctx->r.update_texture(texid, tex); });
}
int atn_update_rendering_config(atn_ctx* ctx, const atn_scene_rendering_config* config)
{
    CTX_OR_FAIL(ctx);
    return guarded(ctx, [&] { return ctx->r.update_rendering_config(config); });
}
int atn_lbvh_rebuild_list(atn_ctx* ctx, uint32_t list_index, uint32_t tri_offset, uint32_t n_triangles, const float* bbox_min, const float* bbox_max)
{
    CTX_OR_FAIL(ctx);
    return guarded(ctx, [&] { return ctx->r.lbvh_rebuild_list(list_index, tri_offset, n_triangles, bbox_min, bbox_max, false); });
}
int atn_lbvh_build(atn_ctx* ctx, const atn_triangle_param* triangles, uint32_t n_triangles, int32_t tri_id_offset,
                   const float* bbox_min, const float* bbox_max, const atn_vec4* vtx_pos, uint32_t n_vertices, int32_t vtx_offset,
                   atn_bvh_node* out_nodes, uint32_t* out_sorted_codes, uint32_t* out_sorted_indices)
{
    CTX_QUIET_OR_FAIL(ctx);
    return guarded(ctx, [&] { return ctx->r.lbvh_build(triangles, n_triangles, tri_id_offset, bbox_min, bbox_max, vtx_pos, n_vertices, vtx_offset,
                                                       out_nodes, out_sorted_codes, out_sorted_indices); });
}
int atn_skin_create(atn_ctx* ctx, const atn_skinning_vertex* vertices, uint32_t n_vertices, uint32_t vtx_offset, uint32_t tri_offset, uint32_t n_triangles,
                    uint32_t n_matrices, atn_skin* out_skin)
{
    CTX_OR_FAIL(ctx);
    return guarded(ctx, [&] { return ctx->r.skin_create(vertices, n_vertices, vtx_offset, tri_offset, n_triangles, n_matrices, out_skin); });
}
int atn_skin_update(atn_ctx* ctx, atn_skin skin, const atn_mat4* matrices, uint32_t n)
{
    CTX_OR_FAIL(ctx);      // enqueued behind the frames in flight, like the other scene updates
    return guarded(ctx, [&] { return ctx->r.skin_update(skin, matrices, n); });
}
int atn_skin_compute(atn_ctx* ctx, atn_skin skin, int32_t is_restart, float* bbox_min, float* bbox_max)
{
    CTX_OR_FAIL(ctx);
    return guarded(ctx, [&] { return ctx->r.skin_compute(skin, is_restart != 0, bbox_min, bbox_max); });
}
int atn_lbvh_rebuild_list_skinned(atn_ctx* ctx, uint32_t list_index, atn_skin skin)
{
    CTX_OR_FAIL(ctx);
    return guarded(ctx, [&] { return ctx->r.lbvh_rebuild_list_skinned(list_index, skin); });
}
int atn_tlas_rebuild(atn_ctx* ctx, const atn_object_param* objects, uint32_t n_objects, const atn_mat4* matrices, uint32_t n_matrices, uint32_t flags)
{
    CTX_OR_FAIL(ctx);      // enqueued behind the frames in flight, like atn_update_tlas
    return guarded(ctx, [&] { return ctx->r.tlas_rebuild(objects, n_objects, matrices, n_matrices, flags); });
}
int atn_tlas_download(atn_ctx* ctx, void* out, uint32_t cap_bytes, uint32_t* out_records, int32_t* out_root_link, uint32_t* out_top_base)
{
    CTX_OR_FAIL(ctx);
    return guarded(ctx, [&] { return ctx->r.tlas_download(out, cap_bytes, out_records, out_root_link, out_top_base); });
}
int atn_skin_download(atn_ctx* ctx, atn_skin skin, int32_t which, void* out_host)
{
    CTX_OR_FAIL(ctx);
    return guarded(ctx, [&] { return ctx->r.skin_download(skin, which, out_host); });
}
int atn_skin_download_list(atn_ctx* ctx, uint32_t list_index, void* out_host, uint32_t capacity_bytes, uint32_t* n_bytes)
{
    CTX_OR_FAIL(ctx);
    return guarded(ctx, [&] { return ctx->r.download_list(list_index, out_host, capacity_bytes, n_bytes); });
}
int atn_skin_destroy(atn_ctx* ctx, atn_skin skin)
{
    CTX_OR_FAIL(ctx);
    return guarded(ctx, [&] { return ctx->r.skin_destroy(skin); });
}
int atn_scene_device_arrays(atn_ctx* ctx, void** vtx_pos, void** vtx_nml, void** triangles)
{
    CTX_QUIET_OR_FAIL(ctx);
    if (!ctx->r.has_scene) return ctx->r.fail(ATN_ERR_NO_SCENE, "atn_upload_scene has not been called");
    // the caller writes these arrays itself from now on: one copy of the scene, updates in place behind the frames in flight
    { int q = ctx->r.quiesce(); if (q) return q; }
    ctx->r.drop_alt_set(); ctx->r.scene_in_place = true;
    if (ctx->r.gm_on) { const int g = ctx->r.set_geometry_motion(0); if (g) return g; }       // (the history cannot follow the caller's writes)
    ctx->r.scene.planar_lights = 0;     // (the caller writes vertices from now on)
    if (vtx_pos) *vtx_pos = ctx->r.vtx_pos.p;
    if (vtx_nml) *vtx_nml = ctx->r.vtx_nml.p;
    if (triangles) *triangles = ctx->r.tris.p;
    return ATN_OK;
}
int atn_set_geometry_motion(atn_ctx* ctx, int32_t on)
{
    CTX_QUIET_OR_FAIL(ctx);
    return guarded(ctx, [&] { return ctx->r.set_geometry_motion(on); });
}
int atn_geometry_motion_stats(atn_ctx* ctx, uint64_t* out3)
{
    CTX_OR_FAIL(ctx);
    if (!out3) return ctx->r.fail(ATN_ERR_INVALID_ARG, "null output");
    for (int k = 0; k < 3; k++) out3[k] = ctx->r.gm_stats[k];
    return ATN_OK;
}
int atn_geometry_motion_matrices(atn_ctx* ctx, float* w2c16, float* prev_w2c16)
{
    CTX_OR_FAIL(ctx);
    if (!w2c16 || !prev_w2c16) return ctx->r.fail(ATN_ERR_INVALID_ARG, "null output");
    if (!ctx->r.gm_stats[0]) return ctx->r.fail(ATN_ERR_INVALID_ARG, "no frame has been rendered with compute_motion = 2");
    std::memcpy(w2c16, ctx->r.gm_w2c, sizeof(ctx->r.gm_w2c)); std::memcpy(prev_w2c16, ctx->r.gm_prev_w2c, sizeof(ctx->r.gm_prev_w2c));
    return ATN_OK;
}
int atn_init_sampler(atn_ctx* ctx, int32_t w, int32_t h, int32_t seed) { CTX_QUIET_OR_FAIL(ctx); return guarded(ctx, [&] { return ctx->r.initSampler(w, h, seed); }); }
int atn_get_random(atn_ctx* ctx, uint32_t* out_host, uint32_t n) { CTX_QUIET_OR_FAIL(ctx); return guarded(ctx, [&] { return ctx->r.getRandom(out_host, n); }); }
uint32_t atn_random_count(atn_ctx* ctx) { return ctx ? ctx->r.n_seeds : 0; }
int atn_set_random(atn_ctx* ctx, const uint32_t* seeds, uint32_t n) { CTX_QUIET_OR_FAIL(ctx); return guarded(ctx, [&] { return ctx->r.setRandom(seeds, n); }); }

int atn_set_screen_shard(atn_ctx* ctx, int32_t rank, int32_t world)
{
    CTX_OR_FAIL(ctx);
    if (world <= 0 || rank < 0 || rank >= world) return ctx->r.fail(ATN_ERR_INVALID_ARG, "bad screen shard");
    ctx->r.rank = rank; ctx->r.world = world;
    return ATN_OK;
}

int atn_render(atn_ctx* ctx, const atn_destination* dst, atn_vec4* out_host) { CTX_OR_FAIL(ctx); return guarded(ctx, [&] { return ctx->r.render(dst, out_host); }); }
int atn_render_burst(atn_ctx* ctx, const atn_destination* dst, int32_t n_frames, atn_vec4* out_host) { CTX_OR_FAIL(ctx); return guarded(ctx, [&] { return ctx->r.render_burst(dst, n_frames, out_host); }); }
int atn_set_regeneration(atn_ctx* ctx, int32_t mode)
{
    CTX_QUIET_OR_FAIL(ctx);
    if (mode < 0 || mode > 1) return ctx->r.fail(ATN_ERR_INVALID_ARG, "regeneration mode out of range");
    ctx->r.regen_mode = mode;
    return ATN_OK;
}
int atn_set_rr_lookahead(atn_ctx* ctx, int32_t mode)
{
    CTX_QUIET_OR_FAIL(ctx);
    if (mode < 0 || mode > 2) return ctx->r.fail(ATN_ERR_INVALID_ARG, "roulette look-ahead mode out of range");
    ctx->r.rr_lookahead = mode;
    return ATN_OK;
}
int32_t atn_rr_lookahead_active(atn_ctx* ctx)
{
    return (ctx && ctx->r.has_scene && ctx->r.rr_lookahead_frame(false)) ? 1 : 0;
}
int atn_rr_lookahead_stats(atn_ctx* ctx, uint64_t out[4])
{
    CTX_OR_FAIL(ctx);
    if (!out) return ctx->r.fail(ATN_ERR_INVALID_ARG, "null output");
    for (int i = 0; i < 4; i++) out[i] = ctx->r.host_stats[8 + i];
    return ATN_OK;
}
int atn_set_nee_deferral(atn_ctx* ctx, int32_t mode)
{
    CTX_QUIET_OR_FAIL(ctx);
    if (mode < 0 || mode > 2) return ctx->r.fail(ATN_ERR_INVALID_ARG, "NEE deferral mode out of range");
    ctx->r.nee_deferral = mode;
    return ATN_OK;
}
int32_t atn_nee_deferral_active(atn_ctx* ctx)
{
    return (ctx && ctx->r.has_scene && ctx->r.nee_deferral_frame(false)) ? 1 : 0;
}
int atn_nee_deferral_stats(atn_ctx* ctx, uint64_t out[2])
{
    CTX_OR_FAIL(ctx);
    if (!out) return ctx->r.fail(ATN_ERR_INVALID_ARG, "null output");
    return guarded(ctx, [&] { return ctx->r.nee_deferral_stats(out); });
}
int atn_set_shade_math(atn_ctx* ctx, int32_t mode)
{
    CTX_QUIET_OR_FAIL(ctx);
    if (mode < 0 || mode > 1) return ctx->r.fail(ATN_ERR_INVALID_ARG, "shade math mode out of range");
    ctx->r.shade_math_relaxed = mode == 1;
    return ATN_OK;
}
int32_t atn_get_regeneration(atn_ctx* ctx) { return ctx ? ctx->r.regen_mode : 0; }
int atn_regen_stage_counts(atn_ctx* ctx, uint32_t* closest, uint32_t* shadow, uint32_t capacity, uint32_t* n_stages)
{
    CTX_QUIET_OR_FAIL(ctx);
    return guarded(ctx, [&] { return ctx->r.regen_stage_counts(closest, shadow, capacity, n_stages); });
}
int atn_reset(atn_ctx* ctx) { CTX_QUIET_OR_FAIL(ctx); return ctx->r.reset(); }
int atn_set_path_batches(atn_ctx* ctx, int32_t n)
{
    CTX_OR_FAIL(ctx);
    if (n < 1 || n > PathTracing::kMaxBatches) return ctx->r.fail(ATN_ERR_INVALID_ARG, "batch count out of range");
    ctx->r.n_batches = n;
    ctx->r.batches_forced = n == 1;     // 1 = strictly serial; larger values stay subject to the size policy
    return ATN_OK;
}

int atn_set_sampling_options(atn_ctx* ctx, int32_t ibl_importance, int32_t tex_bilinear)
{
    CTX_OR_FAIL(ctx);
    return guarded(ctx, [&] { return ctx->r.set_sampling_options(ibl_importance, tex_bilinear); });
}

// texture::at / texture::AtWithBilinear probe (parity tests): n lookups of texture `texid` at uv[2n] -> out[4n]
int atn_sample_texture(atn_ctx* ctx, int32_t texid, uint32_t n, const float* uv_host, float* out_host)
{
    CTX_QUIET_OR_FAIL(ctx);
    PathTracing& r = ctx->r;
    if (!r.has_scene) return r.fail(ATN_ERR_NO_SCENE, "atn_upload_scene has not been called");
    if (texid < 0 || texid >= r.scene.n_textures || n == 0 || !uv_host || !out_host) return r.fail(ATN_ERR_INVALID_ARG, "bad texture id / count");
    return guarded(ctx, [&]() -> int {
        C_HIP(r, hipSetDevice(r.device));
        atn::DevBuf<float> duv, dout;
        C_HIP(r, duv.resize(2 * (size_t)n)); C_HIP(r, dout.resize(4 * (size_t)n));
        C_HIP(r, hipMemcpyAsync(duv.p, uv_host, 8 * (size_t)n, hipMemcpyHostToDevice, r.stream));
        hipLaunchKernelGGL(atn::k_sample_texture, dim3((n + 255) / 256), dim3(256), 0, r.stream, r.scene, texid, n, (const float*)duv.p, dout.p);
        C_HIP(r, hipGetLastError());
        C_HIP(r, hipMemcpyAsync(out_host, dout.p, 16 * (size_t)n, hipMemcpyDeviceToHost, r.stream));
        C_HIP(r, hipStreamSynchronize(r.stream));
        return ATN_OK;
    });
}

int atn_set_frames_in_flight(atn_ctx* ctx, int32_t n)
{
    CTX_OR_FAIL(ctx);
    return guarded(ctx, [&] { return ctx->r.set_frames_in_flight(n); });
}

int atn_bank_streams(atn_ctx* ctx, int32_t* swaps, int32_t* concurrent)
{
    CTX_OR_FAIL(ctx);
    return guarded(ctx, [&] {
        atn::PathTracing& r = ctx->r;
        C_HIP(r, hipSetDevice(r.device));
        { int q = r.quiesce(); if (q) return q; }
        if (swaps) *swaps = r.n_stream_swaps;
        if (concurrent) {
            *concurrent = 1;
            hipStream_t st[atn::PathTracing::kMaxInFlight];
            st[0] = r.stream;
            for (int i = 1; i < r.frames_in_flight; i++) st[i] = r.spare[i - 1].stream;
            for (int i = 0; i < r.frames_in_flight; i++)
                for (int j = 0; j < i; j++) {
                    bool ok = true;
                    if (!atn::streams_run_side_by_side(st[j], st[i], ok)) *concurrent &= ~1;
                    if (!ok) return r.fail(ATN_ERR_HIP, "stream probe failed");
                }
            // bit 1: the side stream, if it was handed out, runs beside every bank stream
            if (r.side_stream) {
                *concurrent |= 2;
                for (int i = 0; i < r.frames_in_flight; i++) {
                    bool ok = true;
                    if (!atn::streams_run_side_by_side(st[i], r.side_stream, ok)) *concurrent &= ~2;
                    if (!ok) return r.fail(ATN_ERR_HIP, "stream probe failed");
                }
            }
        }
        return (int)ATN_OK;
    });
}

int atn_svgf_render(atn_ctx* ctx, const atn_destination* dst, int32_t compute_motion, atn_vec4* out_host, atn_vec4* stages_host)
{
    CTX_OR_FAIL(ctx);
    return guarded(ctx, [&] { return ctx->r.svgf_render(dst, compute_motion, out_host, stages_host); });
}
int atn_svgf_set_motion_depth(atn_ctx* ctx, const atn_vec4* motion_depth, uint32_t n) { CTX_QUIET_OR_FAIL(ctx); return guarded(ctx, [&] { return ctx->r.set_motion_depth(ctx->r.sv_motion, motion_depth, n); }); }
int atn_svgf_reset(atn_ctx* ctx) { CTX_QUIET_OR_FAIL(ctx); return ctx->r.svgf_reset(); }
int atn_svgf_set_atrous_iterations(atn_ctx* ctx, int32_t n)
{
    CTX_OR_FAIL(ctx);
    if (n < 1 || n > 8) return ctx->r.fail(ATN_ERR_INVALID_ARG, "a-trous iteration count out of range");
    ctx->r.sv_atrous_iters = n;
    return ATN_OK;
}
int atn_svgf_set_dilate_temporal_weight(atn_ctx* ctx, int32_t on)
{
    CTX_OR_FAIL(ctx);
    ctx->r.sv_dilate_weight = on ? 1 : 0;
    return ATN_OK;
}
int atn_svgf_download(atn_ctx* ctx, int32_t which, atn_vec4* out_host)
{
    CTX_QUIET_OR_FAIL(ctx);
    PathTracing& r = ctx->r;
    float4* p = r.sv_w > 0 ? r.svgf_buffer(which) : nullptr;
    if (!p || !out_host) return r.fail(ATN_ERR_INVALID_ARG, "no such SVGF buffer (or atn_svgf_render has not run)");
    C_HIP(r, hipSetDevice(r.device));
    C_HIP(r, hipMemcpyAsync(out_host, p, (size_t)r.sv_w * r.sv_h * sizeof(float4), hipMemcpyDeviceToHost, r.stream));
    C_HIP(r, hipStreamSynchronize(r.stream));
    return ATN_OK;
}
int atn_restir_set_options(atn_ctx* ctx, int32_t mode, int32_t n_candidates)
{
    CTX_QUIET_OR_FAIL(ctx);
    return ctx->r.restir_set_options(mode, n_candidates);
}
int atn_restir_render(atn_ctx* ctx, const atn_destination* dst, int32_t compute_motion, atn_vec4* out_host)
{
    CTX_OR_FAIL(ctx);
    return guarded(ctx, [&] { return ctx->r.restir_render(dst, compute_motion, out_host); });
}
int atn_restir_set_motion_depth(atn_ctx* ctx, const atn_vec4* motion_depth, uint32_t n) { CTX_QUIET_OR_FAIL(ctx); return guarded(ctx, [&] { return ctx->r.set_motion_depth(ctx->r.rs_motion, motion_depth, n); }); }
int atn_restir_reset(atn_ctx* ctx) { CTX_QUIET_OR_FAIL(ctx); return ctx->r.restir_reset(); }
int atn_restir_capture(atn_ctx* ctx, int32_t on) { CTX_QUIET_OR_FAIL(ctx); ctx->r.rs_capture = on != 0; return ATN_OK; }
int atn_restir_download(atn_ctx* ctx, int32_t which, void* out_host) { CTX_QUIET_OR_FAIL(ctx); return guarded(ctx, [&] { return ctx->r.restir_download(which, out_host); }); }
int atn_npr_render(atn_ctx* ctx, const atn_destination* dst, atn_vec4* out_host)
{
    CTX_OR_FAIL(ctx);
    return guarded(ctx, [&] { return ctx->r.npr_render(dst, out_host); });
}
int atn_npr_reset(atn_ctx* ctx) { CTX_QUIET_OR_FAIL(ctx); return guarded(ctx, [&] { return ctx->r.npr_reset(); }); }
int atn_npr_capture(atn_ctx* ctx, int32_t on) { CTX_QUIET_OR_FAIL(ctx); ctx->r.np_capture = on != 0; return ATN_OK; }
int atn_npr_download(atn_ctx* ctx, int32_t which, void* out_host) { CTX_QUIET_OR_FAIL(ctx); return guarded(ctx, [&] { return ctx->r.npr_download(which, out_host); }); }
int atn_npr_set_skip_through(atn_ctx* ctx, int32_t mode) { CTX_QUIET_OR_FAIL(ctx); return ctx->r.npr_set_skip_through(mode); }
int atn_npr_advance_download(atn_ctx* ctx, void* out_host) { CTX_QUIET_OR_FAIL(ctx); return guarded(ctx, [&] { return ctx->r.npr_advance_download(out_host); }); }
int atn_volume_render(atn_ctx* ctx, const atn_destination* dst, atn_vec4* out_host)
{
    CTX_OR_FAIL(ctx);
    return guarded(ctx, [&] { return ctx->r.volume_render(dst, out_host); });
}
int atn_volume_set_grids(atn_ctx* ctx, const atn_volume_grid* grids, uint32_t n)
{
    CTX_QUIET_OR_FAIL(ctx);
    return guarded(ctx, [&] { return ctx->r.volume_set_grids(grids, n); });
}
int atn_volume_reset(atn_ctx* ctx) { CTX_QUIET_OR_FAIL(ctx); return guarded(ctx, [&] { return ctx->r.volume_reset(); }); }
int atn_volume_capture(atn_ctx* ctx, int32_t iteration)
{
    CTX_QUIET_OR_FAIL(ctx);
    if (iteration >= atn::kVolIterations) return ctx->r.fail(ATN_ERR_INVALID_ARG, "a path runs 8 iterations: capture 0..7, or < 0 for none");
    ctx->r.vl_capture = iteration < 0 ? -1 : iteration;
    return ATN_OK;
}
int atn_volume_download(atn_ctx* ctx, int32_t which, void* out_host) { CTX_QUIET_OR_FAIL(ctx); return guarded(ctx, [&] { return ctx->r.volume_download(which, out_host); }); }
int atn_volume_phase_table(atn_ctx* ctx, float g, uint32_t n, const float* w, const float* r1, const float* r2, const float* wo, float* out_dir, float* out_eval)
{
    CTX_QUIET_OR_FAIL(ctx);
    return guarded(ctx, [&] { return ctx->r.volume_phase_table(g, n, w, r1, r2, wo, out_dir, out_eval); });
}
int atn_ao_set_params(atn_ctx* ctx, int32_t num_rays, float radius, int32_t filter) { CTX_QUIET_OR_FAIL(ctx); return ctx->r.ao_set_params(num_rays, radius, filter); }
int atn_ao_render(atn_ctx* ctx, const atn_destination* dst, atn_vec4* out_host)
{
    CTX_OR_FAIL(ctx);
    return guarded(ctx, [&] { return ctx->r.ao_render(dst, out_host); });
}
int atn_ao_reset(atn_ctx* ctx) { CTX_QUIET_OR_FAIL(ctx); return guarded(ctx, [&] { return ctx->r.ao_reset(); }); }
int atn_ao_capture(atn_ctx* ctx, int32_t on) { CTX_QUIET_OR_FAIL(ctx); ctx->r.ao_capture = on != 0; return ATN_OK; }
int atn_ao_download(atn_ctx* ctx, int32_t which, void* out_host) { CTX_QUIET_OR_FAIL(ctx); return guarded(ctx, [&] { return ctx->r.ao_download(which, out_host); }); }
int atn_npr_shadow_set_mode(atn_ctx* ctx, int32_t mode) { CTX_QUIET_OR_FAIL(ctx); return ctx->r.ns_set_mode(mode); }
int atn_npr_shadow_download(atn_ctx* ctx, int32_t which, float* out_host, uint32_t n) { CTX_QUIET_OR_FAIL(ctx); return guarded(ctx, [&] { return ctx->r.ns_download(which, out_host, n); }); }
int atn_npr_hatching_set(atn_ctx* ctx, int32_t base, int32_t direction, int32_t ao_num_rays, float ao_radius)
{
    CTX_QUIET_OR_FAIL(ctx);
    return ctx->r.nh_set(base, direction, ao_num_rays, ao_radius);
}
int atn_npr_hatching_get(atn_ctx* ctx, int32_t* base, int32_t* direction, int32_t* ao_num_rays, float* ao_radius)
{
    if (!ctx) return ATN_ERR_INVALID_ARG;
    if (base) *base = ctx->r.nh_base;
    if (direction) *direction = ctx->r.nh_dir;
    if (ao_num_rays) *ao_num_rays = ctx->r.nh_num_rays;
    if (ao_radius) *ao_radius = ctx->r.nh_radius;
    return ATN_OK;
}
int atn_npr_hatching_filter(atn_ctx* ctx, const float* src, const float* depth, int32_t w, int32_t h, int32_t direction, float* out_host)
{
    CTX_QUIET_OR_FAIL(ctx);
    return guarded(ctx, [&] { return ctx->r.nh_filter(src, depth, w, h, direction, out_host); });
}
int atn_npr_hatching_download(atn_ctx* ctx, int32_t which, float* out_host, uint32_t n) { CTX_QUIET_OR_FAIL(ctx); return guarded(ctx, [&] { return ctx->r.nh_download(which, out_host, n); }); }
int atn_npr_shadow_filter(atn_ctx* ctx, const float* lit, const float* depth, int32_t w, int32_t h, float* out_host)
{
    CTX_QUIET_OR_FAIL(ctx);
    return guarded(ctx, [&] { return ctx->r.ns_filter(lit, depth, w, h, out_host); });
}
int atn_svgf_denoise(atn_ctx* ctx, const atn_destination* dst, int32_t compute_motion, atn_vec4* out_host, atn_vec4* stages_host)
{
    CTX_QUIET_OR_FAIL(ctx);
    return guarded(ctx, [&] { return ctx->r.svgf_render(dst, compute_motion, out_host, stages_host, false); });
}
int atn_svgf_upload(atn_ctx* ctx, int32_t which, int32_t width, int32_t height, const atn_vec4* host)
{
    CTX_QUIET_OR_FAIL(ctx);
    PathTracing& r = ctx->r;
    if (!host || width <= 0 || height <= 0) return r.fail(ATN_ERR_INVALID_ARG, "bad SVGF upload");
    C_HIP(r, hipSetDevice(r.device));
    int rc = r.svgf_ensure(width, height, false);
    if (rc) return rc;
    float4* p = r.svgf_buffer(which, true);
    if (!p) return r.fail(ATN_ERR_INVALID_ARG, "no such SVGF buffer");
    C_HIP(r, hipMemcpyAsync(p, host, (size_t)width * height * sizeof(float4), hipMemcpyHostToDevice, r.stream));
    C_HIP(r, hipStreamSynchronize(r.stream));
    if (which == 9) { r.sv_motion.is_set = true; r.sv_motion.count = (size_t)width * height; }
    return ATN_OK;
}
void* atn_svgf_output_device(atn_ctx* ctx) { return ctx ? (void*)ctx->r.sv_out.p : nullptr; }

// the display tail: like atn_svgf_render, atn_taa_resolve does not wait for the frames in flight
int atn_taa_resolve(atn_ctx* ctx, int32_t source, int32_t width, int32_t height, int32_t enable, float gamma, atn_vec4* out_rgba32f, uint32_t* out_rgba8)
{
    CTX_OR_FAIL(ctx);
    return guarded(ctx, [&] { return ctx->r.taa_resolve(source, width, height, enable, gamma, out_rgba32f, out_rgba8); });
}
int atn_taa_upload(atn_ctx* ctx, int32_t which, int32_t width, int32_t height, const atn_vec4* host) { CTX_QUIET_OR_FAIL(ctx); return guarded(ctx, [&] { return ctx->r.taa_upload(which, width, height, host); }); }
int atn_taa_download(atn_ctx* ctx, int32_t which, void* out_host) { CTX_QUIET_OR_FAIL(ctx); return guarded(ctx, [&] { return ctx->r.taa_download(which, out_host); }); }
int atn_taa_reset(atn_ctx* ctx) { CTX_OR_FAIL(ctx); return ctx->r.taa_reset(); }
void* atn_taa_output_device(atn_ctx* ctx) { return (ctx && ctx->r.ta_resolved) ? (void*)ctx->r.ta_hist[ctx->r.ta_pos].p : nullptr; }
void* atn_taa_rgba8_device(atn_ctx* ctx) { return (ctx && ctx->r.ta_resolved) ? (void*)ctx->r.ta_rgba8.p : nullptr; }

void* atn_film_device(atn_ctx* ctx) { return ctx ? (void*)ctx->r.film.p : nullptr; }
void* atn_tile_device(atn_ctx* ctx) { return ctx ? (void*)ctx->r.tile_out.p : nullptr; }
uint32_t atn_tile_slots(atn_ctx* ctx) { return ctx ? ctx->r.n_slots : 0; }
uint32_t atn_planar_area_lights(atn_ctx* ctx) { return (ctx && ctx->r.scene.planar_lights) ? ctx->r.n_planar_lights : 0u; }
uint32_t atn_anyhit_twins(atn_ctx* ctx)
{
    uint32_t n = 0;
    if (ctx) for (const int32_t d : ctx->r.list_twin_delta) n += d != 0 ? 1u : 0u;
    return n;
}
void* atn_stream(atn_ctx* ctx) { return ctx ? (void*)ctx->r.stream : nullptr; }
void* atn_side_stream(atn_ctx* ctx)
{
    if (!ctx) return nullptr;
    try { if (ctx->r.quiesce() != ATN_OK) return nullptr; return (void*)ctx->r.get_side_stream(); } catch (...) { return nullptr; }
}

int atn_synchronize(atn_ctx* ctx)
{
    CTX_QUIET_OR_FAIL(ctx);
    C_HIP(ctx->r, hipStreamSynchronize(ctx->r.stream));
    return ATN_OK;
}

int atn_assemble_tiles(atn_ctx* ctx, const void* gathered_dev, int32_t world, void* film_dev_out)
{
    return atn_assemble_tiles_on(ctx, gathered_dev, world, film_dev_out, nullptr);
}

int atn_assemble_tiles_on(atn_ctx* ctx, const void* gathered_dev, int32_t world, void* film_dev_out, void* hip_stream)
{
    CTX_OR_FAIL(ctx);
    PathTracing& r = ctx->r;
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : r.stream;
    if (!gathered_dev || world <= 0 || r.film_w <= 0) return r.fail(ATN_ERR_INVALID_ARG, "atn_assemble_tiles: nothing rendered yet");
    float4* dst = film_dev_out ? (float4*)film_dev_out : r.film.p;
    const uint32_t total = (uint32_t)world * r.n_slots;
    hipLaunchKernelGGL(atn::k_assemble_tiles, dim3((total + 255) / 256), dim3(256), 0, st,
                       (const float4*)gathered_dev, dst, r.film_w, r.film_h, (r.film_w + 7) / 8, (r.film_h + 7) / 8,
                       world, (int32_t)r.n_slots);
    C_HIP(r, hipGetLastError());
    return ATN_OK;
}

int atn_download_film(atn_ctx* ctx, atn_vec4* out_host)
{
    CTX_QUIET_OR_FAIL(ctx);
    PathTracing& r = ctx->r;
    if (!out_host || !r.film.p) return r.fail(ATN_ERR_INVALID_ARG, "atn_download_film: nothing rendered yet");
    C_HIP(r, hipMemcpyAsync(out_host, r.film.p, (size_t)r.film_w * r.film_h * sizeof(float4), hipMemcpyDeviceToHost, r.stream));
    C_HIP(r, hipStreamSynchronize(r.stream));
    return ATN_OK;
}

// Resume: the film of an earlier run (atn_download_film) becomes the state the next progressive frame continues from --
// FilmProgressive keeps {running mean, sample count in .w} per pixel (src/libaten/renderer/film.cpp:61-71).
int atn_upload_film(atn_ctx* ctx, int32_t width, int32_t height, const atn_vec4* film_host)
{
    CTX_QUIET_OR_FAIL(ctx);
    PathTracing& r = ctx->r;
    if (!film_host || width <= 0 || height <= 0) return r.fail(ATN_ERR_INVALID_ARG, "atn_upload_film: bad size / null film");
    return guarded(ctx, [&]() -> int {
        C_HIP(r, hipSetDevice(r.device));
        C_HIP(r, r.film.resize((size_t)width * height));
        C_HIP(r, hipMemcpyAsync(r.film.p, film_host, (size_t)width * height * sizeof(float4), hipMemcpyHostToDevice, r.stream));
        C_HIP(r, hipStreamSynchronize(r.stream));
        r.film_w = width; r.film_h = height;        // the next render of this size keeps the film instead of clearing it
        return ATN_OK;
    });
}

int atn_download_path_cost(atn_ctx* ctx, uint32_t* out_host)
{
    CTX_QUIET_OR_FAIL(ctx);
    PathTracing& r = ctx->r;
    if (!out_host) return r.fail(ATN_ERR_INVALID_ARG, "null output");
    if (!r.cost_film.p || r.cost_w <= 0) return r.fail(ATN_ERR_INVALID_ARG, "no frame has been rendered with count_stats = 1");
    return guarded(ctx, [&]() -> int {
        if (hipSetDevice(r.device) != hipSuccess) return r.fail(ATN_ERR_HIP, "hipSetDevice");
        if (hipMemcpyAsync(out_host, r.cost_film.p, (size_t)2 * r.cost_w * r.cost_h * sizeof(uint32_t), hipMemcpyDeviceToHost, r.stream) != hipSuccess
            || hipStreamSynchronize(r.stream) != hipSuccess) return r.fail(ATN_ERR_HIP, "cost map download");
        return ATN_OK;
    });
}
int atn_get_stats(atn_ctx* ctx, uint64_t out[8])
{
    CTX_QUIET_OR_FAIL(ctx);
    for (int i = 0; i < 8; i++) out[i] = ctx->r.host_stats[i];
    return ATN_OK;
}

int atn_get_kernel_times(atn_ctx* ctx, float ms[ATN_K_COUNT], uint32_t launches[ATN_K_COUNT])
{
    CTX_QUIET_OR_FAIL(ctx);
    C_HIP(ctx->r, hipStreamSynchronize(ctx->r.stream));
    ctx->r.prof_collect();
    for (int i = 0; i < ATN_K_COUNT; i++) { ms[i] = ctx->r.k_ms[i]; launches[i] = ctx->r.k_launches[i]; }
    return ATN_OK;
}

int atn_reset_kernel_times(atn_ctx* ctx)
{
    CTX_QUIET_OR_FAIL(ctx);
    C_HIP(ctx->r, hipStreamSynchronize(ctx->r.stream));
    ctx->r.prof_collect();
    for (int i = 0; i < ATN_K_MGPU_COUNT; i++) { ctx->r.k_ms[i] = 0; ctx->r.k_launches[i] = 0; }
    return ATN_OK;
}

// ---------------------------------------------------------------- one node, every GPU (host/mgpu.hpp)
int atn_mgpu_create(atn_mgpu** out, const int32_t* devices, int32_t n_devices)
{
    if (!out) return ATN_ERR_INVALID_ARG;
    *out = nullptr;
    atn_mgpu* mg = new (std::nothrow) atn_mgpu();
    if (!mg) return ATN_ERR_OUT_OF_MEMORY;
    int rc = mg_guarded(mg, [&] { return mg->m.init(devices, n_devices); });
    if (rc != ATN_OK) {
        std::fprintf(stderr, "atn_mgpu_create: %s\n", mg->m.last_error.c_str());
        delete mg;
        return rc;
    }
    *out = mg;
    return ATN_OK;
}
void atn_mgpu_destroy(atn_mgpu* mg) { delete mg; }
const char* atn_mgpu_last_error(atn_mgpu* mg) { return mg ? mg->m.last_error.c_str() : "null context"; }
int32_t atn_mgpu_shard_count(atn_mgpu* mg) { return mg ? mg->m.n : 0; }
int32_t atn_mgpu_shard_device(atn_mgpu* mg, int32_t i) { return (mg && i >= 0 && i < mg->m.n) ? mg->m.shard[i]->device : -1; }

int atn_mgpu_upload_scene(atn_mgpu* mg, const atn_scene_desc* scene)
{
    MG_OR_FAIL(mg);
    if (!scene) return mg->m.fail(ATN_ERR_INVALID_ARG, "null scene");
    return mg_guarded(mg, [&] { return mg->m.on_all([&](int i) { return mg->m.shard[i]->UpdateSceneData(scene); }); });
}
int atn_mgpu_update_tlas(atn_mgpu* mg, const atn_object_param* objects, uint32_t n_objects, const atn_mat4* matrices, uint32_t n_matrices,
                         const atn_bvh_node* top_nodes, uint32_t n_top_nodes)
{
    MG_OR_FAIL(mg);
    return mg_guarded(mg, [&] { return mg->m.on_all([&](int i) { return mg->m.shard[i]->updateBVH(objects, n_objects, matrices, n_matrices, top_nodes, n_top_nodes); }); });
}
int atn_mgpu_update_geometry(atn_mgpu* mg, const atn_vec4* vtx_pos, const atn_vec4* vtx_nml, uint32_t n_vertices, uint32_t vtx_offset,
                             const atn_triangle_param* triangles, uint32_t n_triangles, uint32_t tri_offset)
{
    MG_OR_FAIL(mg);
    return mg_guarded(mg, [&] { return mg->m.on_all([&](int i) {
        PathTracing& r = *mg->m.shard[i];
        if (hipSetDevice(r.device) != hipSuccess) return r.fail(ATN_ERR_HIP, "hipSetDevice");
        return r.updateGeometry(vtx_pos, vtx_nml, n_vertices, vtx_offset, triangles, n_triangles, tri_offset); }); });
}
int atn_mgpu_lbvh_rebuild_list(atn_mgpu* mg, uint32_t list_index, uint32_t tri_offset, uint32_t n_triangles, const float* bbox_min, const float* bbox_max)
{
    MG_OR_FAIL(mg);
    return mg_guarded(mg, [&] { return mg->m.on_all([&](int i) {
        PathTracing& r = *mg->m.shard[i];
        if (hipSetDevice(r.device) != hipSuccess) return r.fail(ATN_ERR_HIP, "hipSetDevice");
        return r.lbvh_rebuild_list(list_index, tri_offset, n_triangles, bbox_min, bbox_max, false); }); });
}
int atn_mgpu_tlas_rebuild(atn_mgpu* mg, const atn_object_param* objects, uint32_t n_objects, const atn_mat4* matrices, uint32_t n_matrices, uint32_t flags)
{
    MG_OR_FAIL(mg);
    return mg_guarded(mg, [&] { return mg->m.on_all([&](int i) {
        PathTracing& r = *mg->m.shard[i];
        if (hipSetDevice(r.device) != hipSuccess) return r.fail(ATN_ERR_HIP, "hipSetDevice");
        return r.tlas_rebuild(objects, n_objects, matrices, n_matrices, flags); }); });
}
int atn_mgpu_update_materials(atn_mgpu* mg, const atn_material_param* materials, uint32_t n, uint32_t first)
{
    MG_OR_FAIL(mg);
    return mg_guarded(mg, [&] { return mg->m.on_all([&](int i) { return mg->m.shard[i]->update_materials(materials, n, first); }); });
}
int atn_mgpu_update_lights(atn_mgpu* mg, const atn_light_param* lights, uint32_t n, uint32_t first, int32_t npr_target)
{
    MG_OR_FAIL(mg);
    return mg_guarded(mg, [&] { return mg->m.on_all([&](int i) { return mg->m.shard[i]->update_lights(lights, n, first, npr_target); }); });
}
int atn_mgpu_update_texture(atn_mgpu* mg, int32_t texid, const atn_texture_desc* tex)
{
    MG_OR_FAIL(mg);
    return mg_guarded(mg, [&] { return mg->m.on_all([&](int i) { return mg->m.shard[i]->update_texture(texid, tex); }); });
}
int atn_mgpu_update_rendering_config(atn_mgpu* mg, const atn_scene_rendering_config* config)
{
    MG_OR_FAIL(mg);
    return mg_guarded(mg, [&] { return mg->m.on_all([&](int i) { return mg->m.shard[i]->update_rendering_config(config); }); });
}
int atn_mgpu_update_camera(atn_mgpu* mg, const atn_camera_param* camera)
{
    MG_OR_FAIL(mg);
    for (auto& s : mg->m.shard) { int rc = s->updateCamera(camera); if (rc) return mg->m.fail(rc, s->last_error); }
    return ATN_OK;
}
int atn_mgpu_init_sampler(atn_mgpu* mg, int32_t w, int32_t h, int32_t seed)
{
    MG_OR_FAIL(mg);
    return mg_guarded(mg, [&]() -> int {
        if (w <= 0 || h <= 0) return mg->m.fail(ATN_ERR_INVALID_ARG, "bad sampler size");
        std::vector<uint32_t> v((size_t)w * h);         // one mt19937 pass, shared by every shard (seeds are global)
        std::mt19937 src(seed);
        for (auto& x : v) x = (uint32_t)src();
        return mg->m.on_all([&](int i) { return mg->m.shard[i]->setRandom(v.data(), (uint32_t)v.size()); });
    });
}
int atn_mgpu_set_random(atn_mgpu* mg, const uint32_t* seeds, uint32_t n)
{
    MG_OR_FAIL(mg);
    return mg_guarded(mg, [&] { return mg->m.on_all([&](int i) { return mg->m.shard[i]->setRandom(seeds, n); }); });
}
int atn_mgpu_render(atn_mgpu* mg, const atn_destination* dst, atn_vec4* out_host)
{
    MG_OR_FAIL(mg);
    return mg_guarded(mg, [&] { return mg->m.render(dst, out_host); });
}
int atn_mgpu_render_burst(atn_mgpu* mg, const atn_destination* dst, int32_t n_frames, atn_vec4* out_host)
{
    MG_OR_FAIL(mg);
    return mg_guarded(mg, [&] { return mg->m.render_burst(dst, n_frames, out_host); });
}
int atn_mgpu_set_regeneration(atn_mgpu* mg, int32_t mode)
{
    MG_OR_FAIL(mg);
    if (mode < 0 || mode > 1) return mg->m.fail(ATN_ERR_INVALID_ARG, "regeneration mode out of range");
    return mg_guarded(mg, [&] {
        int rc = mg->m.synchronize();
        if (rc) return rc;
        for (int i = 0; i < mg->m.n; i++) mg->m.shard[i]->regen_mode = mode;
        return (int)ATN_OK;
    });
}
int atn_mgpu_set_sphere_intersection(atn_mgpu* mg, int32_t mode)
{
    MG_OR_FAIL(mg);
    if (mode < 0 || mode > 1) return mg->m.fail(ATN_ERR_INVALID_ARG, "sphere intersection mode out of range");
    return mg_guarded(mg, [&] {
        for (int i = 0; i < mg->m.n; i++) mg->m.shard[i]->sphere_mode = mode;
        return (int)ATN_OK;
    });
}
int atn_mgpu_reset(atn_mgpu* mg)
{
    MG_OR_FAIL(mg);
    return mg_guarded(mg, [&] { return mg->m.on_all([&](int i) { return mg->m.shard[i]->reset(); }); });
}
int atn_mgpu_synchronize(atn_mgpu* mg) { MG_OR_FAIL(mg); return mg_guarded(mg, [&] { return mg->m.synchronize(); }); }
int atn_mgpu_set_frames_in_flight(atn_mgpu* mg, int32_t n)
{
    MG_OR_FAIL(mg);
    return mg_guarded(mg, [&] { return mg->m.on_all([&](int i) { return mg->m.shard[i]->set_frames_in_flight(n); }); });
}
// node-wide SVGF (MultiGpu::svgf_render): the filters, their settings and their planes live on shard 0
int atn_mgpu_svgf_render(atn_mgpu* mg, const atn_destination* dst, int32_t compute_motion, atn_vec4* out_host, atn_vec4* stages_host)
{
    MG_OR_FAIL(mg);
    return mg_guarded(mg, [&] { return mg->m.svgf_render(dst, compute_motion, out_host, stages_host); });
}
int atn_mgpu_svgf_set_motion_depth(atn_mgpu* mg, const atn_vec4* motion_depth, uint32_t n)
{
    MG_OR_FAIL(mg);
    return mg_guarded(mg, [&]() -> int {
        int rc = mg->m.synchronize();
        if (rc) return rc;
        PathTracing& r = *mg->m.shard[0];
        rc = r.set_motion_depth(r.sv_motion, motion_depth, n);
        return rc ? mg->m.fail(rc, "shard 0: " + r.last_error) : (int)ATN_OK;
    });
}
int atn_mgpu_svgf_reset(atn_mgpu* mg) { MG_OR_FAIL(mg); return mg_guarded(mg, [&] { return mg->m.svgf_reset(); }); }
int atn_mgpu_svgf_set_atrous_iterations(atn_mgpu* mg, int32_t n)
{
    MG_OR_FAIL(mg);
    if (n < 1 || n > 8) return mg->m.fail(ATN_ERR_INVALID_ARG, "a-trous iteration count out of range");
    mg->m.shard[0]->sv_atrous_iters = n;
    return ATN_OK;
}
int atn_mgpu_svgf_set_dilate_temporal_weight(atn_mgpu* mg, int32_t on)
{
    MG_OR_FAIL(mg);
    mg->m.shard[0]->sv_dilate_weight = on ? 1 : 0;
    return ATN_OK;
}
int atn_mgpu_svgf_download(atn_mgpu* mg, int32_t which, atn_vec4* out_host)
{
    MG_OR_FAIL(mg);
    return mg_guarded(mg, [&]() -> int {
        atn::MultiGpu& m = mg->m;
        int rc = m.synchronize();
        if (rc) return rc;
        PathTracing& r = *m.shard[0];
        float4* p = r.sv_w > 0 ? r.svgf_buffer(which) : nullptr;
        if (!p || !out_host) return m.fail(ATN_ERR_INVALID_ARG, "no such SVGF buffer (or atn_mgpu_svgf_render has not run)");
        if (hipSetDevice(r.device) != hipSuccess
            || hipMemcpyAsync(out_host, p, (size_t)r.sv_w * r.sv_h * sizeof(float4), hipMemcpyDeviceToHost, r.stream) != hipSuccess
            || hipStreamSynchronize(r.stream) != hipSuccess) return m.fail(ATN_ERR_HIP, "SVGF plane download failed");
        return ATN_OK;
    });
}
void* atn_mgpu_svgf_output_device(atn_mgpu* mg) { return mg ? (void*)mg->m.shard[0]->sv_out.p : nullptr; }
int atn_mgpu_get_kernel_times(atn_mgpu* mg, int32_t shard, float ms[ATN_K_MGPU_COUNT], uint32_t launches[ATN_K_MGPU_COUNT])
{
    MG_OR_FAIL(mg);
    return mg_guarded(mg, [&]() -> int {
        atn::MultiGpu& m = mg->m;
        if (shard < 0 || shard >= m.n || !ms || !launches) return m.fail(ATN_ERR_INVALID_ARG, "atn_mgpu_get_kernel_times: no such shard");
        int rc = m.synchronize();
        if (rc) return rc;
        PathTracing& r = *m.shard[shard];
        if (hipSetDevice(r.device) != hipSuccess) return m.fail(ATN_ERR_HIP, "hipSetDevice");
        r.prof_collect();
        for (int i = 0; i < ATN_K_MGPU_COUNT; i++) { ms[i] = r.k_ms[i]; launches[i] = r.k_launches[i]; }
        return ATN_OK;
    });
}
int atn_mgpu_reset_kernel_times(atn_mgpu* mg)
{
    MG_OR_FAIL(mg);
    return mg_guarded(mg, [&]() -> int {
        atn::MultiGpu& m = mg->m;
        int rc = m.synchronize();
        if (rc) return rc;
        for (auto& s : m.shard) {
            if (hipSetDevice(s->device) != hipSuccess) return m.fail(ATN_ERR_HIP, "hipSetDevice");
            s->prof_collect();
            for (int i = 0; i < ATN_K_MGPU_COUNT; i++) { s->k_ms[i] = 0; s->k_launches[i] = 0; }
        }
        return ATN_OK;
    });
}
void* atn_mgpu_film_device(atn_mgpu* mg) { return mg ? (void*)mg->m.full.p : nullptr; }
int atn_mgpu_download_film(atn_mgpu* mg, atn_vec4* out_host)
{
    MG_OR_FAIL(mg);
    atn::MultiGpu& m = mg->m;
    if (!out_host || !m.full.p || m.width <= 0) return m.fail(ATN_ERR_INVALID_ARG, "atn_mgpu_download_film: nothing rendered yet");
    if (hipSetDevice(m.shard[0]->device) != hipSuccess
        || hipMemcpyAsync(out_host, m.full.p, (size_t)m.width * m.height * sizeof(float4), hipMemcpyDeviceToHost, m.comm) != hipSuccess
        || hipStreamSynchronize(m.comm) != hipSuccess) return m.fail(ATN_ERR_HIP, "film download failed");
    return ATN_OK;
}

// ---------------------------------------------------------------- stage entry points
int atn_generate_paths(atn_ctx* ctx, int32_t width, int32_t height, int32_t sample, uint32_t frame, atn_ray* out_host)
{
    CTX_QUIET_OR_FAIL(ctx);
    PathTracing& r = ctx->r;
    if (!r.has_camera || r.n_seeds == 0 || !out_host) return r.fail(ATN_ERR_INVALID_ARG, "atn_generate_paths: camera / sampler / output missing");
    C_HIP(r, hipSetDevice(r.device));
    const int32_t sr = r.rank, sw = r.world;
    r.rank = 0; r.world = 1;
    int rc = r.ensure_frame(width, height, 1);
    if (rc) { r.rank = sr; r.world = sw; return rc; }
    atn_destination d{}; d.width = width; d.height = height; d.maxDepth = 1; d.russianRouletteDepth = 1; d.sample = 1; d.frame = frame;
    atn::FrameParams fp = r.frame_params(d);
    fp.sample = sample;
    atn::PathBuffers pb = r.buffers(false);
    atn::DevBuf<atn_ray> out;
    C_HIP(r, out.resize((size_t)width * height));
    C_HIP(r, hipMemsetAsync(r.counters.p, 0, (size_t)4 * r.counters_depth * 4, r.stream));
    if (sample > 0) C_HIP(r, hipMemsetAsync(r.done.p, 0, (size_t)r.n_slots * 4, r.stream));
    hipLaunchKernelGGL(atn::k_gen_path, dim3(atn::grid_for(r.n_slots)), dim3(256), 0, r.stream, pb, fp, r.camera, (const uint32_t*)r.seeds.p);
    hipLaunchKernelGGL(atn::k_export_rays, dim3((r.n_slots + 255) / 256), dim3(256), 0, r.stream, pb, fp, out.p);
    C_HIP(r, hipMemcpyAsync(out_host, out.p, (size_t)width * height * sizeof(atn_ray), hipMemcpyDeviceToHost, r.stream));
    C_HIP(r, hipStreamSynchronize(r.stream));
    r.rank = sr; r.world = sw;      // (the next render re-validates its path buffers against its own shard's slot count)
    return ATN_OK;
}

int atn_trace_closest(atn_ctx* ctx, const atn_ray* rays_host, uint32_t n, float t_min, float t_max,
                      atn_intersection* out_host, uint64_t* stats_out)
{
    CTX_QUIET_OR_FAIL(ctx);
    PathTracing& r = ctx->r;
    if (!r.has_scene) return r.fail(ATN_ERR_NO_SCENE, "atn_upload_scene has not been called");
    if (!rays_host || !out_host) return r.fail(ATN_ERR_INVALID_ARG, "null rays / output");
    if (n == 0) { if (stats_out) { stats_out[0] = stats_out[1] = 0; } return ATN_OK; }
    C_HIP(r, hipSetDevice(r.device));
    atn::DevBuf<atn_ray> rays; atn::DevBuf<atn_intersection> out; atn::DevBuf<unsigned long long> st;
    C_HIP(r, rays.resize(n)); C_HIP(r, out.resize(n)); C_HIP(r, st.resize(8));
    C_HIP(r, hipMemcpyAsync(rays.p, rays_host, (size_t)n * sizeof(atn_ray), hipMemcpyHostToDevice, r.stream));
    C_HIP(r, hipMemsetAsync(st.p, 0, 64, r.stream));
    {
        // the probe exercises the walk the scene's tree calls for (or the forced one), whatever n is
        const bool refill = r.refill_walk(false);
        const dim3 g(r.trace_grid(n, refill)), t(refill ? (uint32_t)atn::kTraceBlock : 256u);
        const atn_ray* rp = rays.p;
        if (r.n_sphere_leaves) atn::sph_launch_batch(stats_out != nullptr, refill, g.x, t.x, r.stream, r.scene, rp, n, t_min, t_max, out.p, st.p);
        else atn::with_flags([&](auto c, auto rf) {
            hipLaunchKernelGGL((atn::k_trace_batch<decltype(c)::value, decltype(rf)::value>), g, t, 0, r.stream, r.scene, rp, n, t_min, t_max, out.p, st.p);
        }, stats_out != nullptr, refill);
    }
    C_HIP(r, hipGetLastError());
    C_HIP(r, hipMemcpyAsync(out_host, out.p, (size_t)n * sizeof(atn_intersection), hipMemcpyDeviceToHost, r.stream));
    unsigned long long hs[8] = {};
    C_HIP(r, hipMemcpyAsync(hs, st.p, 64, hipMemcpyDeviceToHost, r.stream));
    C_HIP(r, hipStreamSynchronize(r.stream));
    if (stats_out) { stats_out[0] = hs[3]; stats_out[1] = hs[4]; }
    return ATN_OK;
}

int atn_trace_shadow(atn_ctx* ctx, const atn_shadow_query* queries_host, uint32_t n, int32_t flavour, uint8_t* out_visible)
{
    CTX_QUIET_OR_FAIL(ctx);
    PathTracing& r = ctx->r;
    if (!r.has_scene) return r.fail(ATN_ERR_NO_SCENE, "atn_upload_scene has not been called");
    if (flavour < atn::kShadowProbeFused || flavour > atn::kShadowProbeRegen) return r.fail(ATN_ERR_INVALID_ARG, "atn_trace_shadow: unknown flavour");
    if (n == 0) return ATN_OK;
    if (!queries_host || !out_visible) return r.fail(ATN_ERR_INVALID_ARG, "null queries / output");
    if (r.scene.n_lights <= 0) return r.fail(ATN_ERR_UNSUPPORTED, "atn_trace_shadow: the scene has no lights");
    if (r.n_sphere_leaves && (flavour == atn::kShadowProbeDeferred || flavour == atn::kShadowProbeRegen)) return r.sph_refuse("atn_trace_shadow: only the fused and the counted flavour test sphere leaves");
    if (r.n_sphere_leaves && r.scene.any_alpha) return r.sph_refuse("shadow rays do not look through alpha / stencil materials in a scene with sphere leaves");
    for (uint32_t i = 0; i < n; i++)
        if (queries_host[i].light < 0 || queries_host[i].light >= r.scene.n_lights) return r.fail(ATN_ERR_INVALID_ARG, "atn_trace_shadow: light index outside the scene's lights");
    const uint64_t slots64 = 2ull * n + atn::kShadowProbePad;
    if (slots64 > atn::kShadowSlotMask) return r.fail(ATN_ERR_UNSUPPORTED, "atn_trace_shadow: more than 2^25 queries");
    const uint32_t n_slots = (uint32_t)slots64;
    C_HIP(r, hipSetDevice(r.device));
    // the queue: every used slot once, in a fixed shuffled order (Fisher-Yates over a 64-bit LCG)
    std::vector<uint32_t> queue(n);
    for (uint32_t i = 0; i < n; i++) queue[i] = 2u * i + 1u;
    uint64_t lcg = 0x9e3779b97f4a7c15ull;
    for (uint32_t i = n - 1u; i > 0u; i--) {
        lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
        std::swap(queue[i], queue[(uint32_t)((lcg >> 33) % (uint64_t)(i + 1u))]);
    }
    const bool deferred = flavour == atn::kShadowProbeDeferred, regen = flavour == atn::kShadowProbeRegen, counted = flavour == atn::kShadowProbeCounted;
    atn::DevBuf<atn_shadow_query> dq; atn::DevBuf<float4> sh_o, sh_d, sh_c, contrib, pend; atn::DevBuf<uint32_t> shadow_q, flags, counters, errs;
    atn::DevBuf<unsigned long long> stats; atn::DevBuf<uint8_t> out;
    C_HIP(r, dq.resize(n)); C_HIP(r, sh_o.resize(n_slots)); C_HIP(r, sh_d.resize(n_slots)); C_HIP(r, sh_c.resize(n_slots)); C_HIP(r, contrib.resize(n_slots));
    C_HIP(r, shadow_q.resize(n_slots)); C_HIP(r, counters.resize(4)); C_HIP(r, errs.resize(4)); C_HIP(r, out.resize(n));
    if (regen) C_HIP(r, pend.resize(n_slots));
    if (deferred) C_HIP(r, flags.resize(n_slots));
    if (counted) { C_HIP(r, stats.resize(16)); C_HIP(r, hipMemsetAsync(stats.p, 0, 128, r.stream)); }
    C_HIP(r, hipMemcpyAsync(dq.p, queries_host, (size_t)n * sizeof(atn_shadow_query), hipMemcpyHostToDevice, r.stream));
    C_HIP(r, hipMemcpyAsync(shadow_q.p, queue.data(), (size_t)n * 4, hipMemcpyHostToDevice, r.stream));
    const uint32_t hc[4] = { 0u, n, 0u, 0u };       // q_count[0], sh_count[0] = n, the two fetch cursors cleared
    C_HIP(r, hipMemcpyAsync(counters.p, hc, 16, hipMemcpyHostToDevice, r.stream));
    C_HIP(r, hipMemsetAsync(errs.p, 0, 16, r.stream));
    atn::PathBuffers pb{};
    pb.sh_o = sh_o.p; pb.sh_d = sh_d.p; pb.sh_c = sh_c.p; pb.contrib = contrib.p; pb.shadow_q = shadow_q.p;
    pb.q_count = counters.p; pb.sh_count = counters.p + 1; pb.fetch_closest = counters.p + 2; pb.fetch_shadow = counters.p + 3;
    pb.pend = pend.p; pb.nee_reached = flags.p; pb.stats = stats.p;
    const dim3 g_slots((n_slots + 255u) / 256u), t256(256);
    hipLaunchKernelGGL(atn::k_shadow_probe_fill, g_slots, t256, 0, r.stream, pb, (const atn_shadow_query*)dq.p, n, n_slots, flavour);
    {
        // the walk the scene's tree calls for (or the forced one), whatever n is -- as atn_trace_closest picks it; everything else of the
        // launch is the pass's own plan
        atn::PassPlan plan = r.plan_pass(regen ? atn::PassKind::Regen : atn::PassKind::Serial, n);
        plan.refill = r.refill_walk(false);
        plan.trace_grid = r.trace_grid(n, plan.refill);
        plan.fused_grid = r.trace_grid(2u * n, plan.refill);
        if (counted) r.launch_trace<true>(plan, pb, true, 0, r.stream);
        else {
            const atn::TraceLaunch tl = atn::trace_launch(plan, 1);     // (a stage behind the first: the launch that carries shadow rays)
            if (regen) atn::regen_launch_trace(tl, r.stream, pb, r.scene, 0, -1, 0);
            else atn::launch_trace_fused<false>(tl, r.stream, pb, r.scene, 0, -1, 0);
        }
    }
    C_HIP(r, hipGetLastError());
    hipLaunchKernelGGL(atn::k_shadow_probe_check, g_slots, t256, 0, r.stream, pb, (const atn_shadow_query*)dq.p, n, n_slots, flavour, out.p, errs.p);
    C_HIP(r, hipGetLastError());
    uint32_t he[4] = {};
    C_HIP(r, hipMemcpyAsync(out_visible, out.p, n, hipMemcpyDeviceToHost, r.stream));
    C_HIP(r, hipMemcpyAsync(he, errs.p, 16, hipMemcpyDeviceToHost, r.stream));
    C_HIP(r, hipStreamSynchronize(r.stream));
    if (he[0] || he[1] || he[2])
        return r.fail(ATN_ERR_HIP, "atn_trace_shadow: " + std::to_string(he[0]) + " unused slots changed, " + std::to_string(he[1]) + " ray records changed, "
                                   + std::to_string(he[2]) + " result records hold neither verdict");
    return ATN_OK;
}

int atn_shade_stage(atn_ctx* ctx, const atn_shade_call* call, const atn_shade_vertex* records_host, uint32_t n, atn_shade_result* out_host)
{
    CTX_QUIET_OR_FAIL(ctx);
    PathTracing& r = ctx->r;
    if (!r.has_scene) return r.fail(ATN_ERR_NO_SCENE, "atn_upload_scene has not been called");
    if (!call) return r.fail(ATN_ERR_INVALID_ARG, "atn_shade_stage: null call");
    if (call->flavour != 0 && call->flavour != 1) return r.fail(ATN_ERR_INVALID_ARG, "atn_shade_stage: unknown flavour");
    const bool svgf = call->flavour == 1;
    if (call->chunk_items < 0 || call->chunk_items > atn::kChunkItems) return r.fail(ATN_ERR_INVALID_ARG, "atn_shade_stage: chunk_items outside 0..4");
    if (call->queue_order < 0 || call->queue_order > 1) return r.fail(ATN_ERR_INVALID_ARG, "atn_shade_stage: unknown queue order");
    if (call->width <= 0 || call->height <= 0 || call->max_depth <= 0 || call->sample < 0) return r.fail(ATN_ERR_INVALID_ARG, "atn_shade_stage: bad frame");
    if (call->bounce < 0 || call->bounce >= call->max_depth) return r.fail(ATN_ERR_INVALID_ARG, "atn_shade_stage: bounce outside 0 .. max_depth - 1");
    if (!r.has_camera || r.n_seeds == 0) return r.fail(ATN_ERR_INVALID_ARG, "atn_shade_stage: camera / sampler missing");
    if (r.shade_math_relaxed) return r.fail(ATN_ERR_UNSUPPORTED, "atn_shade_stage: the relaxed-math kernel is not the parity path: atn_set_shade_math(0)");
    { const int sr = r.sph_refuse("atn_shade_stage's records have no sphere hits"); if (sr) return sr; }
    if (n == 0) return ATN_OK;
    if (!records_host || !out_host) return r.fail(ATN_ERR_INVALID_ARG, "null records / output");
    C_HIP(r, hipSetDevice(r.device));
    const int32_t sr = r.rank, sw = r.world;
    r.rank = 0; r.world = 1;        // (the whole frame's slots, as atn_generate_paths)
    struct Restore { PathTracing& r; int32_t rank, world; ~Restore() { r.rank = rank; r.world = world; } } restore{ r, sr, sw };
    int rc = r.ensure_frame(call->width, call->height, call->max_depth);
    if (rc) return rc;
    const uint32_t n_slots = r.n_slots;
    // record -> the slot its pixel owns (slot_to_pixel's inverse: 8 x 8 tiles); pixels distinct and inside the frame, hit records inside the scene
    const int32_t tiles_x = (call->width + 7) / 8;
    std::vector<int32_t> rec_of(n_slots, -1);
    std::vector<uint32_t> queue(n);
    const uint32_t known = atn::F_TERMINATED | atn::F_SINGULAR | atn::F_HIT | atn::F_LAST_SPECULAR;
    const size_t n_tris = r.n_scene_tris < r.tris.n ? r.n_scene_tris : r.tris.n;
    for (uint32_t i = 0; i < n; i++) {
        const atn_shade_vertex& v = records_host[i];
        if (v.pixel < 0 || (int64_t)v.pixel >= (int64_t)call->width * call->height) return r.fail(ATN_ERR_INVALID_ARG, "atn_shade_stage: a pixel outside the frame");
        if ((v.flags & ~known) || (v.flags & atn::F_TERMINATED)) return r.fail(ATN_ERR_INVALID_ARG, "atn_shade_stage: a record that is terminated or carries unknown flag bits");
        if (v.objid >= 0 && ((size_t)v.objid >= r.objects.n || v.tri_id < 0 || (size_t)v.tri_id >= n_tris
                             || !(v.a >= -1.0F && v.a <= 2.0F && v.b >= -1.0F && v.b <= 2.0F)))
            return r.fail(ATN_ERR_INVALID_ARG, "atn_shade_stage: a hit record outside the scene");
        const int32_t x = v.pixel % call->width, y = v.pixel / call->width;
        const uint32_t slot = (uint32_t)((y / 8) * tiles_x + x / 8) * 64u + (uint32_t)((y & 7) * 8 + (x & 7));
        if (slot >= n_slots) return r.fail(ATN_ERR_INVALID_ARG, "atn_shade_stage: a pixel outside the frame");
        if (rec_of[slot] >= 0) return r.fail(ATN_ERR_INVALID_ARG, "atn_shade_stage: two records share a pixel");
        rec_of[slot] = (int32_t)i;
        queue[i] = slot;
    }
    if (call->queue_order == 0) {       // a fixed shuffle (Fisher-Yates over a 64-bit LCG), as atn_trace_shadow's
        uint64_t lcg = 0x9e3779b97f4a7c15ull;
        for (uint32_t i = n - 1u; i > 0u; i--) {
            lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
            std::swap(queue[i], queue[(uint32_t)((lcg >> 33) % (uint64_t)(i + 1u))]);
        }
    }
    atn_destination d{}; d.width = call->width; d.height = call->height; d.maxDepth = call->max_depth; d.russianRouletteDepth = call->rr_depth;
    d.sample = 1; d.frame = call->frame;
    atn::FrameParams fp = r.frame_params(d);
    fp.sample = call->sample;
    atn::PathBuffers pb = r.buffers(false);
    // the launch the renderer would make for n live paths: its plan, its flavour; chunk_items forced where the caller asks
    atn::PassPlan plan = r.plan_pass(svgf ? atn::PassKind::Svgf : atn::PassKind::Serial, n);
    if (call->chunk_items) {
        plan.shade_items = call->chunk_items;
        plan.shade_grid = atn::grid_for((n + (uint32_t)plan.shade_items - 1u) / (uint32_t)plan.shade_items);
    }
    fp.chunk_items = plan.shade_items;
    atn::DevBuf<atn_shade_vertex> drec; atn::DevBuf<atn_shade_result> dout; atn::DevBuf<int32_t> drec_of; atn::DevBuf<uint32_t> dqueue, seen, errs;
    C_HIP(r, drec.resize(n)); C_HIP(r, dout.resize(n)); C_HIP(r, drec_of.resize(n_slots)); C_HIP(r, dqueue.resize(n)); C_HIP(r, seen.resize(n_slots)); C_HIP(r, errs.resize(4));
    // "svgf": three AOV planes of the probe's own, a texel per pixel -- the context needs no SVGF frame behind it -- and the fourth row
    // of W2C as SVGFRenderer's frame computes it from the camera (FrameMatrices::advance on a fresh pair of matrices)
    atn::DevBuf<float4> aov_nd, aov_am, aov_primary;
    atn::SvgfShade sv{};
    const uint32_t n_pixels = (uint32_t)call->width * (uint32_t)call->height;
    if (svgf) {
        C_HIP(r, aov_nd.resize(n_pixels)); C_HIP(r, aov_am.resize(n_pixels)); C_HIP(r, aov_primary.resize(n_pixels));
        sv.nd = aov_nd.p; sv.am = aov_am.p; sv.primary = aov_primary.p;
        atn::FrameMatrices fm; float w2c[16];
        fm.advance(r.camera);
        atn::mat_mul(fm.V2C, fm.W2V, w2c);
        sv.w2c3[0] = w2c[12]; sv.w2c3[1] = w2c[13]; sv.w2c3[2] = w2c[14]; sv.w2c3[3] = w2c[15];
    }
    C_HIP(r, hipMemcpyAsync(drec.p, records_host, (size_t)n * sizeof(atn_shade_vertex), hipMemcpyHostToDevice, r.stream));
    C_HIP(r, hipMemcpyAsync(drec_of.p, rec_of.data(), (size_t)n_slots * 4, hipMemcpyHostToDevice, r.stream));
    C_HIP(r, hipMemcpyAsync(dqueue.p, queue.data(), (size_t)n * 4, hipMemcpyHostToDevice, r.stream));
    C_HIP(r, hipMemsetAsync(seen.p, 0, (size_t)n_slots * 4, r.stream));
    C_HIP(r, hipMemsetAsync(errs.p, 0, 16, r.stream));
    C_HIP(r, hipMemsetAsync(r.counters.p, 0, (size_t)4 * r.counters_depth * 4, r.stream));
    C_HIP(r, hipMemcpyAsync(pb.q_count + call->bounce, &n, 4, hipMemcpyHostToDevice, r.stream));
    const dim3 g_slots((n_slots + 255u) / 256u), t256(256);
    hipLaunchKernelGGL(atn::k_shade_probe_fill, g_slots, t256, 0, r.stream, pb, (const atn_shade_vertex*)drec.p, (const int32_t*)drec_of.p,
                       (const uint32_t*)dqueue.p, n, n_slots, call->bounce, sv, n_pixels);
    C_HIP(r, hipGetLastError());
    if (svgf) r.launch_shade<true>(plan, r.stream, pb, fp, call->bounce, sv);
    else r.launch_shade<false>(plan, r.stream, pb, fp, call->bounce, atn::SvgfShade{});
    C_HIP(r, hipGetLastError());
    hipLaunchKernelGGL(atn::k_shade_probe_queues, g_slots, t256, 0, r.stream, pb, (const int32_t*)drec_of.p, (const uint32_t*)dqueue.p, n, n_slots,
                       call->bounce, (int32_t)r.counters_depth, seen.p, errs.p);
    hipLaunchKernelGGL(atn::k_shade_probe_check, g_slots, t256, 0, r.stream, pb, (const atn_shade_vertex*)drec.p, (const int32_t*)drec_of.p, n_slots,
                       (const uint32_t*)seen.p, dout.p, errs.p, sv, n_pixels, call->width);
    C_HIP(r, hipGetLastError());
    uint32_t he[4] = {};
    C_HIP(r, hipMemcpyAsync(out_host, dout.p, (size_t)n * sizeof(atn_shade_result), hipMemcpyDeviceToHost, r.stream));
    C_HIP(r, hipMemcpyAsync(he, errs.p, 16, hipMemcpyDeviceToHost, r.stream));
    C_HIP(r, hipStreamSynchronize(r.stream));
    if (he[0] || he[1] || he[2] || he[3])
        return r.fail(ATN_ERR_HIP, "atn_shade_stage: " + std::to_string(he[0]) + " unused slots changed, " + std::to_string(he[1])
                                   + " planes changed that a vertex leaves alone, " + std::to_string(he[2]) + " slots queued twice, "
                                   + std::to_string(he[3]) + " queue entries that were not handed in");
    return ATN_OK;
}

int atn_cmj_samples(atn_ctx* ctx, uint32_t index, uint32_t dimension, uint32_t scramble, int32_t n, float* out_host)
{
    CTX_QUIET_OR_FAIL(ctx);
    PathTracing& r = ctx->r;
    if (n <= 0 || !out_host) return r.fail(ATN_ERR_INVALID_ARG, "bad sample count");
    C_HIP(r, hipSetDevice(r.device));
    atn::DevBuf<float> out;
    C_HIP(r, out.resize(n));
    hipLaunchKernelGGL(atn::k_cmj_samples, dim3(1), dim3(64), 0, r.stream, index, dimension, scramble, n, out.p);
    C_HIP(r, hipMemcpyAsync(out_host, out.p, (size_t)n * 4, hipMemcpyDeviceToHost, r.stream));
    C_HIP(r, hipStreamSynchronize(r.stream));
    return ATN_OK;
}

int atn_cmj_batch(atn_ctx* ctx, uint32_t n, const uint32_t* index, const uint32_t* dimension, const uint32_t* scramble,
                  int32_t draws, float* out_host)
{
    CTX_QUIET_OR_FAIL(ctx);
    PathTracing& r = ctx->r;
    if (n == 0 || draws <= 0 || !index || !dimension || !scramble || !out_host) return r.fail(ATN_ERR_INVALID_ARG, "bad cmj batch");
    C_HIP(r, hipSetDevice(r.device));
    atn::DevBuf<uint32_t> di, dd, ds; atn::DevBuf<float> out;
    C_HIP(r, di.resize(n)); C_HIP(r, dd.resize(n)); C_HIP(r, ds.resize(n)); C_HIP(r, out.resize((size_t)n * draws));
    C_HIP(r, hipMemcpyAsync(di.p, index, 4 * (size_t)n, hipMemcpyHostToDevice, r.stream));
    C_HIP(r, hipMemcpyAsync(dd.p, dimension, 4 * (size_t)n, hipMemcpyHostToDevice, r.stream));
    C_HIP(r, hipMemcpyAsync(ds.p, scramble, 4 * (size_t)n, hipMemcpyHostToDevice, r.stream));
    hipLaunchKernelGGL(atn::k_cmj_batch, dim3((n + 255) / 256), dim3(256), 0, r.stream, n, (const uint32_t*)di.p,
                       (const uint32_t*)dd.p, (const uint32_t*)ds.p, (int)draws, out.p);
    C_HIP(r, hipGetLastError());
    C_HIP(r, hipMemcpyAsync(out_host, out.p, 4 * (size_t)n * draws, hipMemcpyDeviceToHost, r.stream));
    C_HIP(r, hipStreamSynchronize(r.stream));
    return ATN_OK;
}

int atn_ray_offset(atn_ctx* ctx, uint32_t n, const float* origins, const float* normals, float* out_host)
{
    CTX_QUIET_OR_FAIL(ctx);
    PathTracing& r = ctx->r;
    if (n == 0 || !origins || !normals || !out_host) return r.fail(ATN_ERR_INVALID_ARG, "bad ray offset batch");
    C_HIP(r, hipSetDevice(r.device));
    atn::DevBuf<float> o, nm, out;
    C_HIP(r, o.resize(3 * (size_t)n)); C_HIP(r, nm.resize(3 * (size_t)n)); C_HIP(r, out.resize(3 * (size_t)n));
    C_HIP(r, hipMemcpyAsync(o.p, origins, 12 * (size_t)n, hipMemcpyHostToDevice, r.stream));
    C_HIP(r, hipMemcpyAsync(nm.p, normals, 12 * (size_t)n, hipMemcpyHostToDevice, r.stream));
    hipLaunchKernelGGL(atn::k_ray_offset, dim3((n + 255) / 256), dim3(256), 0, r.stream, n, (const float*)o.p, (const float*)nm.p, out.p);
    C_HIP(r, hipGetLastError());
    C_HIP(r, hipMemcpyAsync(out_host, out.p, 12 * (size_t)n, hipMemcpyDeviceToHost, r.stream));
    C_HIP(r, hipStreamSynchronize(r.stream));
    return ATN_OK;
}

int atn_libm_probe(atn_ctx* ctx, int32_t kind, uint32_t n, const float* a, const float* b, float* out_host)
{
    CTX_QUIET_OR_FAIL(ctx);
    PathTracing& r = ctx->r;
    if (n == 0 || !a || !b || !out_host || kind < 0 || kind > 10) return r.fail(ATN_ERR_INVALID_ARG, "bad libm probe");
    C_HIP(r, hipSetDevice(r.device));
    atn::DevBuf<float> da, db, out;
    C_HIP(r, da.resize(n)); C_HIP(r, db.resize(n)); C_HIP(r, out.resize(n));
    C_HIP(r, hipMemcpyAsync(da.p, a, 4 * (size_t)n, hipMemcpyHostToDevice, r.stream));
    C_HIP(r, hipMemcpyAsync(db.p, b, 4 * (size_t)n, hipMemcpyHostToDevice, r.stream));
    hipLaunchKernelGGL(atn::k_libm_probe, dim3((n + 255) / 256), dim3(256), 0, r.stream, kind, n, (const float*)da.p, (const float*)db.p, out.p);
    C_HIP(r, hipGetLastError());
    C_HIP(r, hipMemcpyAsync(out_host, out.p, 4 * (size_t)n, hipMemcpyDeviceToHost, r.stream));
    C_HIP(r, hipStreamSynchronize(r.stream));
    return ATN_OK;
}

int atn_material_table(atn_ctx* ctx, int32_t mtrl_id, uint32_t n, const float* nrm, const float* wi,
                       const uint32_t* index, const uint32_t* dimension, const uint32_t* scramble, const float* uv,
                       float* out_sample, float* out_eval)
{
    CTX_QUIET_OR_FAIL(ctx);
    PathTracing& r = ctx->r;
    if (!r.has_scene) return r.fail(ATN_ERR_NO_SCENE, "atn_upload_scene has not been called");
    if (mtrl_id < 0 || mtrl_id >= r.scene.n_materials || n == 0) return r.fail(ATN_ERR_INVALID_ARG, "bad material id / count");
    C_HIP(r, hipSetDevice(r.device));
    atn::DevBuf<float> dn, dw, duv, ds, de; atn::DevBuf<uint32_t> di, dsc, ddim;
    C_HIP(r, dn.resize(3 * (size_t)n)); C_HIP(r, dw.resize(3 * (size_t)n)); C_HIP(r, duv.resize(2 * (size_t)n));
    C_HIP(r, ds.resize(7 * (size_t)n)); C_HIP(r, de.resize(5 * (size_t)n)); C_HIP(r, di.resize(n)); C_HIP(r, dsc.resize(n));
    if (dimension) { C_HIP(r, ddim.resize(n)); C_HIP(r, hipMemcpyAsync(ddim.p, dimension, 4 * (size_t)n, hipMemcpyHostToDevice, r.stream)); }
    C_HIP(r, hipMemcpyAsync(dn.p, nrm, 12 * (size_t)n, hipMemcpyHostToDevice, r.stream));
    C_HIP(r, hipMemcpyAsync(dw.p, wi, 12 * (size_t)n, hipMemcpyHostToDevice, r.stream));
    C_HIP(r, hipMemcpyAsync(duv.p, uv, 8 * (size_t)n, hipMemcpyHostToDevice, r.stream));
    C_HIP(r, hipMemcpyAsync(di.p, index, 4 * (size_t)n, hipMemcpyHostToDevice, r.stream));
    C_HIP(r, hipMemcpyAsync(dsc.p, scramble, 4 * (size_t)n, hipMemcpyHostToDevice, r.stream));
    hipLaunchKernelGGL(atn::k_material_table, dim3((n + 63) / 64), dim3(64), 0, r.stream, r.scene, mtrl_id, n,
                       (const float*)dn.p, (const float*)dw.p, (const uint32_t*)di.p, (const uint32_t*)(dimension ? ddim.p : nullptr), (const uint32_t*)dsc.p, (const float*)duv.p, ds.p, de.p);
    C_HIP(r, hipGetLastError());
    C_HIP(r, hipMemcpyAsync(out_sample, ds.p, 28 * (size_t)n, hipMemcpyDeviceToHost, r.stream));
    C_HIP(r, hipMemcpyAsync(out_eval, de.p, 20 * (size_t)n, hipMemcpyDeviceToHost, r.stream));
    C_HIP(r, hipStreamSynchronize(r.stream));
    return ATN_OK;
}

int atn_material_eval(atn_ctx* ctx, int32_t mtrl_id, uint32_t n, const float* nrm, const float* wi, const float* wo, const float* uv, float* out_eval)
{
    CTX_QUIET_OR_FAIL(ctx);
    PathTracing& r = ctx->r;
    if (!r.has_scene) return r.fail(ATN_ERR_NO_SCENE, "atn_upload_scene has not been called");
    if (mtrl_id < 0 || mtrl_id >= r.scene.n_materials || n == 0) return r.fail(ATN_ERR_INVALID_ARG, "bad material id / count");
    if (!nrm || !wi || !wo || !uv || !out_eval) return r.fail(ATN_ERR_INVALID_ARG, "null argument");
    return guarded(ctx, [&]() -> int {
        C_HIP(r, hipSetDevice(r.device));
        atn::DevBuf<float> dn, dw, dwo, duv, de;
        C_HIP(r, dn.resize(3 * (size_t)n)); C_HIP(r, dw.resize(3 * (size_t)n)); C_HIP(r, dwo.resize(3 * (size_t)n));
        C_HIP(r, duv.resize(2 * (size_t)n)); C_HIP(r, de.resize(5 * (size_t)n));
        C_HIP(r, hipMemcpyAsync(dn.p, nrm, 12 * (size_t)n, hipMemcpyHostToDevice, r.stream));
        C_HIP(r, hipMemcpyAsync(dw.p, wi, 12 * (size_t)n, hipMemcpyHostToDevice, r.stream));
        C_HIP(r, hipMemcpyAsync(dwo.p, wo, 12 * (size_t)n, hipMemcpyHostToDevice, r.stream));
        C_HIP(r, hipMemcpyAsync(duv.p, uv, 8 * (size_t)n, hipMemcpyHostToDevice, r.stream));
        hipLaunchKernelGGL(atn::k_material_eval, dim3((n + 255) / 256), dim3(256), 0, r.stream, r.scene, mtrl_id, n,
                           (const float*)dn.p, (const float*)dw.p, (const float*)dwo.p, (const float*)duv.p, de.p);
        C_HIP(r, hipGetLastError());
        C_HIP(r, hipMemcpyAsync(out_eval, de.p, 20 * (size_t)n, hipMemcpyDeviceToHost, r.stream));
        C_HIP(r, hipStreamSynchronize(r.stream));
        return ATN_OK;
    });
}

int atn_compact2(atn_ctx* ctx, const int32_t* flags_a_host, const int32_t* flags_b_host, uint32_t n, uint32_t grid_blocks,
                 int32_t* out_a_host, uint32_t* out_count_a, int32_t* out_b_host, uint32_t* out_count_b)
{
    CTX_QUIET_OR_FAIL(ctx);
    PathTracing& r = ctx->r;
    if (!flags_a_host || !out_a_host || !out_count_a) return r.fail(ATN_ERR_INVALID_ARG, "null argument");
    if (flags_b_host && (!out_b_host || !out_count_b)) return r.fail(ATN_ERR_INVALID_ARG, "null output for the second queue");
    *out_count_a = 0;
    if (out_count_b) *out_count_b = 0;
    if (n == 0) return ATN_OK;
    return guarded(ctx, [&]() -> int {
        C_HIP(r, hipSetDevice(r.device));
        atn::DevBuf<int32_t> fa, fb; atn::DevBuf<uint32_t> oa, ob, c;
        C_HIP(r, fa.resize(n)); C_HIP(r, oa.resize(n)); C_HIP(r, c.resize(2));
        C_HIP(r, hipMemcpyAsync(fa.p, flags_a_host, 4 * (size_t)n, hipMemcpyHostToDevice, r.stream));
        if (flags_b_host) {
            C_HIP(r, fb.resize(n)); C_HIP(r, ob.resize(n));
            C_HIP(r, hipMemcpyAsync(fb.p, flags_b_host, 4 * (size_t)n, hipMemcpyHostToDevice, r.stream));
        }
        C_HIP(r, hipMemsetAsync(c.p, 0, 8, r.stream));
        uint32_t grid = grid_blocks ? grid_blocks : atn::grid_for((n + (uint32_t)atn::kChunkItems - 1u) / (uint32_t)atn::kChunkItems);
        hipLaunchKernelGGL(atn::k_compact_append, dim3(grid), dim3(256), 0, r.stream, (const int32_t*)fa.p, (const int32_t*)fb.p, n,
                           oa.p, c.p, ob.p, c.p + 1);
        C_HIP(r, hipGetLastError());
        uint32_t hc[2] = { 0, 0 };
        C_HIP(r, hipMemcpyAsync(hc, c.p, 8, hipMemcpyDeviceToHost, r.stream));
        C_HIP(r, hipStreamSynchronize(r.stream));
        if (hc[0] > n || hc[1] > n) return r.fail(ATN_ERR_HIP, "queue append reserved more entries than exist");
        *out_count_a = hc[0];
        if (hc[0]) C_HIP(r, hipMemcpyAsync(out_a_host, oa.p, 4 * (size_t)hc[0], hipMemcpyDeviceToHost, r.stream));
        if (flags_b_host) {
            *out_count_b = hc[1];
            if (hc[1]) C_HIP(r, hipMemcpyAsync(out_b_host, ob.p, 4 * (size_t)hc[1], hipMemcpyDeviceToHost, r.stream));
        }
        C_HIP(r, hipStreamSynchronize(r.stream));
        return ATN_OK;
    });
}

int atn_compact(atn_ctx* ctx, const int32_t* flags_host, uint32_t n, int32_t* out_idx_host, uint32_t* out_count)
{
    // the product's unordered block append, put into index order on the host: the entries ARE the indices, so the
    // sorted queue is the stable compaction
    int rc = atn_compact2(ctx, flags_host, nullptr, n, 0, out_idx_host, out_count, nullptr, nullptr);
    if (rc == ATN_OK && *out_count) std::sort(out_idx_host, out_idx_host + *out_count);
    return rc;
}

uint32_t atn_sizeof_scene_desc(void) { return (uint32_t)sizeof(atn_scene_desc); }
uint32_t atn_sizeof_destination(void) { return (uint32_t)sizeof(atn_destination); }
// what this binary was built from: aten_amd.build.kernel_sources_sha16() of the sources + the extra compile flags, passed in by
// the build recipe (aten_amd/build.py, tools/build_variants.sh).  bench.py uses PMC records only for the binary they were taken on.
#ifndef ATN_BUILD_ID
#define ATN_BUILD_ID "unknown"
#endif
const char* atn_build_id(void) { return ATN_BUILD_ID; }
uint32_t atn_abi_version(void) { return 4; }     // 4: atn_bank_streams' *concurrent is a bit mask (bit 0 = banks overlap, bit 1 = the side stream does) since r05; r06 adds atn_set_regeneration / atn_render_burst / atn_regen_stage_counts / atn_set_upload_options / atn_mgpu_render_burst
//     // 3: atn_material_table takes the starting dimension, atn_compact3 dropped (r04); 2: atn_scene_desc grew the NPR fields, atn_toon_param spelled out (r02)

} // extern "C"
