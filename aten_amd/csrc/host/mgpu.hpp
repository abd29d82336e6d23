// One-node multi-GPU renderer behind the C-ABI (atn_mgpu_*, include/aten_amd.h).
//
// The reference's GPU renderer is single-device (idaten::Renderer, src/libidaten/kernel/renderer.h:17-179, driven from
// one window thread: src/device_renderer/main.cpp:133-149,196-204).  A C++ aten application that wants every GPU of the
// node keeps that call shape -- UpdateSceneData once, render(dst) per frame -- and this object does the rest:
//
//   * one atn::PathTracing per shard, each with its own host WORKER THREAD (kernel launches of 8 devices are not
//     serialised through one thread; a frame is ~13 launches per device);
//   * the scene is replicated (it is << 288 GB), the screen is cut into 8x8 tiles, tile t -> shard t % N
//     (atn_set_screen_shard), seeds and pixel indices stay global, so the image does not depend on N;
//   * the only exchange of a frame: every shard PUSHES its tile buffer into the gather buffer on device 0 with a peer
//     copy over xGMI on its own stream (33 MB per 1080p frame in total, 7/8 of it crossing links, each over a different
//     link into device 0), then device 0 scatters the gathered tiles into the full frame (k_assemble_tiles).  Two
//     gather buffers + events both ways: frame f + 1 renders while frame f is being assembled, no host
//     synchronisation inside a frame unless the caller asks for the film in host memory.
//
// No collective library is needed for a gather-to-one of this size; bench.py's one-process-per-GPU mode uses RCCL's
// all_gather for the same exchange (every rank gets the frame).
//
// A device ordinal may appear several times in the shard list: the shards then share that GPU.  That is how the whole
// N > 1 path (threads, shards, peer copies, events, assembly) is exercised on a one-GPU box.
#pragma once
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>

namespace atn {

class Worker {
public:
    Worker() : th_([this] { loop(); }) {}
    ~Worker()
    {
        { std::lock_guard<std::mutex> g(m_); quit_ = true; }
        cv_.notify_all();
        th_.join();
    }
    void post(std::function<int()> f)
    {
        { std::lock_guard<std::mutex> g(m_); job_ = std::move(f); has_job_ = true; done_ = false; }
        cv_.notify_all();
    }
    int wait()
    {
        std::unique_lock<std::mutex> g(m_);
        cv_.wait(g, [this] { return done_; });
        return rc_;
    }

private:
    void loop()
    {
        for (;;) {
            std::function<int()> f;
            {
                std::unique_lock<std::mutex> g(m_);
                cv_.wait(g, [this] { return has_job_ || quit_; });
                if (quit_ && !has_job_) return;
                f = std::move(job_);
                has_job_ = false;
            }
            int rc;
            try { rc = f(); }
            catch (const std::bad_alloc&) { rc = ATN_ERR_OUT_OF_MEMORY; }
            catch (...) { rc = ATN_ERR_INVALID_ARG; }
            { std::lock_guard<std::mutex> g(m_); rc_ = rc; done_ = true; }
            cv_.notify_all();
        }
    }
    std::mutex m_;
    std::condition_variable cv_;
    std::function<int()> job_;
    bool has_job_ = false, done_ = true, quit_ = false;
    int rc_ = 0;
    std::thread th_;        // last member: the thread starts after everything it touches exists
};

class MultiGpu {
public:
    std::string last_error;
    std::vector<std::unique_ptr<PathTracing>> shard;
    std::vector<std::unique_ptr<Worker>> worker;
    int n = 0;

    // exchange state, all on shard 0's device
    DevStream comm;
    DevBuf<float4> gathered[2], full;
    DevEvent ev_pushed[2][PathTracing::kMaxShards];         // shard i's tiles of the frame using buffer k have arrived
    DevEvent ev_assembled[2];                                // buffer k has been scattered into `full`
    bool assembled_recorded[2] = { false, false };
    uint64_t frames = 0;
    int32_t width = 0, height = 0;

    int fail(int code, const std::string& msg) { last_error = msg; return code; }

    int init(const int32_t* devices, int32_t count)
    {
        int visible = 0;
        if (hipGetDeviceCount(&visible) != hipSuccess || visible <= 0)
            return fail(ATN_ERR_NO_DEVICE, "no HIP device available (libaten_amd has no CPU fallback)");
        std::vector<int32_t> list;
        if (devices && count > 0) list.assign(devices, devices + count);
        else {
            const int32_t want = count > 0 ? count : visible;
            if (want > visible) return fail(ATN_ERR_INVALID_ARG, "more devices requested than visible");
            for (int32_t i = 0; i < want; i++) list.push_back(i);
        }
        if (list.empty() || list.size() > (size_t)PathTracing::kMaxShards) return fail(ATN_ERR_INVALID_ARG, "shard count out of range");
        n = (int)list.size();
        for (int i = 0; i < n; i++) {
            shard.emplace_back(new PathTracing());
            int rc = shard[i]->init(list[i]);
            if (rc != ATN_OK) return fail(rc, shard[i]->last_error);
            shard[i]->rank = i; shard[i]->world = n;
            worker.emplace_back(new Worker());
        }
        const int d0 = shard[0]->device;
        for (int i = 1; i < n; i++) {
            const int di = shard[i]->device;
            if (di == d0) continue;
            int can = 0;
            (void)hipDeviceCanAccessPeer(&can, di, d0);
            if (can) {
                (void)hipSetDevice(di);
                hipError_t e = hipDeviceEnablePeerAccess(d0, 0);
                if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) return fail(ATN_ERR_HIP, std::string("hipDeviceEnablePeerAccess: ") + hipGetErrorString(e));
                (void)hipGetLastError();
            }       // otherwise hipMemcpyPeerAsync stages through host memory: slower, still correct
        }
        ATN_HIP(hipSetDevice(d0));
        ATN_HIP(hipStreamCreateWithFlags(&comm.h, hipStreamNonBlocking));
        for (int k = 0; k < 2; k++) {
            ATN_HIP(hipEventCreateWithFlags(&ev_assembled[k].h, hipEventDisableTiming));
            for (int i = 0; i < n; i++) {
                ATN_HIP(hipSetDevice(shard[i]->device));
                ATN_HIP(hipEventCreateWithFlags(&ev_pushed[k][i].h, hipEventDisableTiming));
            }
        }
        return ATN_OK;
    }

    ~MultiGpu()
    {
        worker.clear();     // joins the threads; the events and `comm` go with their wrappers, before the shards
        if (!shard.empty()) (void)hipSetDevice(shard[0]->device);
        gathered[0].release(); gathered[1].release(); full.release();
    }

    // run f(i) on every shard's worker thread, wait for all; first failure wins
    int on_all(const std::function<int(int)>& f)
    {
        for (int i = 0; i < n; i++) worker[i]->post([&f, i] { return f(i); });
        int rc = ATN_OK, who = -1;
        for (int i = 0; i < n; i++) {
            const int r = worker[i]->wait();
            if (r != ATN_OK && rc == ATN_OK) { rc = r; who = i; }
        }
        if (rc != ATN_OK) last_error = "shard " + std::to_string(who) + ": " + shard[who]->last_error;
        return rc;
    }

    // ≙ idaten::PathTracing::render for the whole node.  Returns once everything is ENQUEUED (or, with out_host,
    // once the frame is in host memory).
    int render(const atn_destination* d, atn_vec4* out_host) { return render_burst(d, 1, out_host); }

    // n_frames consecutive frames on every shard (atn_render_burst: one regenerated pool per shard when regeneration is on), then ONE
    // exchange: the progressive film is only looked at after the burst, so its tiles travel once per burst, not once per frame.
    int render_burst(const atn_destination* d, int32_t n_frames, atn_vec4* out_host)
    {
        if (!d || d->width <= 0 || d->height <= 0) return fail(ATN_ERR_INVALID_ARG, "bad destination");
        if (n_frames <= 0) return fail(ATN_ERR_INVALID_ARG, "bad burst length");
        const int k = (int)(frames & 1u);
        const int d0 = shard[0]->device;
        const size_t px = (size_t)d->width * d->height;
        ATN_HIP(hipSetDevice(d0));
        if (d->width != width || d->height != height) {
            ATN_HIP(hipStreamSynchronize(comm));
            ATN_HIP(full.resize(px));
            ATN_HIP(hipMemsetAsync(full.p, 0, px * sizeof(float4), comm));
            width = d->width; height = d->height;
        }
        float4* gbuf[2] = { nullptr, nullptr };
        {
            const uint32_t tiles = (uint32_t)((d->width + 7) / 8) * (uint32_t)((d->height + 7) / 8);
            const size_t slots = (size_t)((tiles + n - 1) / n) * 64;
            for (int b = 0; b < 2; b++) { ATN_HIP(gathered[b].resize(slots * n)); gbuf[b] = gathered[b].p; }
        }
        const bool wait_assembled = assembled_recorded[k];
        int rc = on_all([&](int i) -> int {
            PathTracing& r = *shard[i];
            int rr = n_frames == 1 ? r.render(d, nullptr) : r.render_burst(d, n_frames, nullptr);
            if (rr != ATN_OK) return rr;
            // push this shard's tiles into slot i of the gather buffer on device 0 (peer copy on the shard's stream)
            if (wait_assembled) { if (hipStreamWaitEvent(r.stream, ev_assembled[k], 0) != hipSuccess) return r.fail(ATN_ERR_HIP, "hipStreamWaitEvent"); }
            const size_t bytes = (size_t)r.n_slots * sizeof(float4);
            hipError_t e = (r.device == d0)
                ? hipMemcpyAsync(gbuf[k] + (size_t)i * r.n_slots, r.tile_out.p, bytes, hipMemcpyDeviceToDevice, r.stream)
                : hipMemcpyPeerAsync(gbuf[k] + (size_t)i * r.n_slots, d0, r.tile_out.p, r.device, bytes, r.stream);
            if (e == hipSuccess) e = hipEventRecord(ev_pushed[k][i], r.stream);
            if (e != hipSuccess) return r.fail(ATN_ERR_HIP, std::string("tile push: ") + hipGetErrorString(e));
            return ATN_OK;
        });
        if (rc != ATN_OK) return rc;
        ATN_HIP(hipSetDevice(d0));
        for (int i = 0; i < n; i++) ATN_HIP(hipStreamWaitEvent(comm, ev_pushed[k][i], 0));
        const uint32_t total = (uint32_t)n * shard[0]->n_slots;
        hipLaunchKernelGGL(k_assemble_tiles, dim3((total + 255) / 256), dim3(256), 0, comm, (const float4*)gbuf[k], full.p,
                           d->width, d->height, (d->width + 7) / 8, (d->height + 7) / 8, n, (int32_t)shard[0]->n_slots);
        ATN_HIP(hipGetLastError());
        ATN_HIP(hipEventRecord(ev_assembled[k], comm));
        assembled_recorded[k] = true;
        frames++;
        if (out_host) {
            ATN_HIP(hipMemcpyAsync(out_host, full.p, px * sizeof(float4), hipMemcpyDeviceToHost, comm));
            ATN_HIP(hipStreamSynchronize(comm));
        }
        return ATN_OK;
    }

    // ------------------------------------------------------------------------------------------------
    // Node-wide SVGF (atn_mgpu_svgf_*, docs/MGPU_SVGF.md).  The path pass is most of an SVGF frame and no path reads another pixel's
    // state, so it shards like the plain path tracer; the filters gather over neighbourhoods that cross tiles, so they run on ONE
    // GPU over the whole frame (gather the colour and AOV planes, then denoise).  Per frame:
    //   1. every shard's worker runs PathTracing::svgf_path_half on its tiles: the shard's pixels of slot k of its hand-over planes
    //      (contributions, normal+depth, albedo+id, primary positions);
    //   2. shards 1 .. N-1 pack those pixels (k_svgf_pack_tiles: four planes, slot-major) and push the buffer into gather buffer k
    //      on device 0 -- one peer copy per shard, on the stream the shard's path half ran on;
    //   3. device 0 scatters the gathered buffers into shard 0's hand-over planes of slot k (k_svgf_unpack_tiles, one launch);
    //   4. shard 0 runs PathTracing::svgf_filter_half behind that.
    // Shard 0 neither packs nor pushes: its pixels are in place, and the unpack's thread grid starts at rank 1, so no pixel of a
    // plane has two writers.  Everything is ordered by events; the host waits only where atn_svgf_render itself does (a size
    // change, a host pointer).  The hazards, each handled where the comment `hazard` stands below:
    //   (a) gather buffer k is overwritten by frame f's pushes only after the unpack of frame f - 2 has read it (ev_sv_unpacked[k]:
    //       the ev_assembled pattern of render_burst);
    //   (b) the unpack writes slot k of shard 0's hand-over planes, whose last reader was k_svgf_temporal of frame f - 2;
    //   (c) the filter half needs both shard 0's own path half and the unpack;
    //   (d) with frames in flight a shard's consecutive frames run on different bank streams: its packed buffer (one per slot) and
    //       slot k of its hand-over planes are reused by frame f + 2 only after frame f's pack and push have completed;
    //   (e) a size change reallocates planes and buffers that frames in flight may still use.
    // Gather buffer k on device 0: [rank][plane][slot] float4, rank 0's part unused; k is the frame's hand-over slot, which the
    // shards advance in lockstep (after a failure they may not: the caller resets, atn_mgpu_svgf_reset).
    DevBuf<float4> sv_gathered[2];
    DevEvent ev_sv_pushed[2][PathTracing::kMaxShards];      // shard i's packed planes of the frame using gather buffer k have arrived
    DevEvent ev_sv_unpacked[2];                              // gather buffer k has been scattered into shard 0's planes
    bool sv_unpacked_recorded[2] = { false, false };
    bool sv_events_ready = false;
    int32_t sv_gw = 0, sv_gh = 0;

    int svgf_render(const atn_destination* d, int32_t compute_motion, atn_vec4* out_host, atn_vec4* stages_host)
    {
        PathTracing& r0 = *shard[0];
        const int d0 = r0.device;
        // the refusals shard 0 would make, before any shard has moved
        int rc = r0.check_ready(d);
        if (rc) return fail(rc, "shard 0: " + r0.last_error);
        for (int i = 0; i < n; i++)
            if (shard[i]->n_sphere_leaves) { const int sr = shard[i]->sph_refuse("the SVGF renderer does not trace sphere leaves"); return fail(sr, "shard " + std::to_string(i) + ": " + shard[i]->last_error); }
        if (compute_motion == 2)
            return fail(ATN_ERR_UNSUPPORTED, "atn_mgpu_svgf_render: compute_motion = 2 is not supported: the geometry history (previous positions of the "
                                             "deforming meshes, per-pixel primary hit ids) has no node-wide form yet; use compute_motion = 1 or atn_svgf_render");
        const size_t px = (size_t)d->width * d->height;
        if (!compute_motion && (!r0.sv_motion.is_set || r0.sv_motion.count < px))
            return fail(ATN_ERR_INVALID_ARG, "no motion/depth buffer: call atn_mgpu_svgf_set_motion_depth or pass compute_motion = 1");
        for (int i = 1; i < n; i++) shard[i]->sv_handover_only = true;
        ATN_HIP(hipSetDevice(d0));
        if (!sv_events_ready) {
            for (int k = 0; k < 2; k++) {
                ATN_HIP(hipSetDevice(d0));
                ATN_HIP(hipEventCreateWithFlags(&ev_sv_unpacked[k].h, hipEventDisableTiming));
                for (int i = 1; i < n; i++) {
                    ATN_HIP(hipSetDevice(shard[i]->device));
                    ATN_HIP(hipEventCreateWithFlags(&ev_sv_pushed[k][i].h, hipEventDisableTiming));
                }
            }
            ATN_HIP(hipSetDevice(d0));
            sv_events_ready = true;
        }
        const uint32_t tiles = (uint32_t)((d->width + 7) / 8) * (uint32_t)((d->height + 7) / 8);
        const uint32_t slots = ((tiles + (uint32_t)n - 1u) / (uint32_t)n) * 64u;     // PathTracing::ensure_frame's n_slots, the same on every shard
        if (d->width != sv_gw || d->height != sv_gh) {
            // hazard (e): every shard idle before anything is resized (each shard's path half quiesces its own streams on a size
            // change too, but a shard's push into device 0's gather buffer is not among shard 0's streams)
            rc = synchronize();
            if (rc) return rc;
            sv_unpacked_recorded[0] = sv_unpacked_recorded[1] = false;
            ATN_HIP(hipSetDevice(d0));
            if (n > 1) for (int k = 0; k < 2; k++) ATN_HIP(sv_gathered[k].resize((size_t)n * kSvgfGatherPlanes * slots));
            sv_gw = d->width; sv_gh = d->height;
        }
        const bool stages = stages_host != nullptr, prof = d->profile != 0;
        const GatherLaunch gl = svgf_gather_launch(slots, n);
        rc = on_all([&](int i) -> int {
            PathTracing& r = *shard[i];
            int rr = r.svgf_path_half(d, compute_motion, i == 0 && stages, true);
            if (rr != ATN_OK || i == 0) return rr;
            if (r.n_slots != slots) return r.fail(ATN_ERR_INVALID_ARG, "slot count differs from the node's (internal)");
            const int k = r.sv_pass.slot;
            const SvgfFrame& sf = r.sv_pass.sf;
            hipStream_t st = r.stream;      // the bank stream this frame's path half ran on: pack and push go behind it
            hipError_t e = r.sv_packed[k].resize((size_t)kSvgfGatherPlanes * slots);
            if (e != hipSuccess) return r.fail(ATN_ERR_HIP, std::string("packed planes: ") + hipGetErrorString(e));
            // hazard (d): packed buffer k was last read by the push of frame f - 2, on another bank's stream when frames are in
            // flight.  The path half above already waited for that push on `st` (r.sv_ev_prepare[k], recorded below), so the
            // pack behind it may overwrite the buffer; with one frame in flight all of it is on one stream.
            r.prof_begin(prof, ATN_K_SVGF_PACK, st);
            hipLaunchKernelGGL(k_svgf_pack_tiles, dim3(gl.pack_grid), dim3(256), 0, st, (const float4*)sf.contribs, (const float4*)sf.g_nd,
                               (const float4*)sf.g_am, (const float4*)sf.primary, r.sv_packed[k].p, d->width, d->height, i, n, slots);
            r.prof_end(prof);
            e = hipGetLastError();
            // hazard (a): gather buffer k still holds frame f - 2's planes until that frame's unpack has read them
            if (e == hipSuccess && sv_unpacked_recorded[k]) e = hipStreamWaitEvent(st, ev_sv_unpacked[k], 0);
            const size_t count = (size_t)kSvgfGatherPlanes * slots, bytes = count * sizeof(float4);
            float4* dst = sv_gathered[k].p + (size_t)i * count;
            if (e == hipSuccess) e = (r.device == d0) ? hipMemcpyAsync(dst, r.sv_packed[k].p, bytes, hipMemcpyDeviceToDevice, st)
                                                      : hipMemcpyPeerAsync(dst, d0, r.sv_packed[k].p, r.device, bytes, st);
            if (e == hipSuccess) e = hipEventRecord(ev_sv_pushed[k][i], st);
            // hazard (d), the other end: slot k of this shard's hand-over planes and packed buffer k are free again once this
            // push has completed -- the event the path half of frame f + 2 waits for in front of its paths (on shard 0 the
            // filter half records it behind k_svgf_temporal instead)
            if (e == hipSuccess && r.sv_pass.pipelined) { e = hipEventRecord(r.sv_ev_prepare[k], st); r.sv_prepare_recorded[k] = true; }
            if (e != hipSuccess) return r.fail(ATN_ERR_HIP, std::string("plane push: ") + hipGetErrorString(e));
            return ATN_OK;
        });
        if (rc != ATN_OK) return rc;
        ATN_HIP(hipSetDevice(d0));
        const int k = r0.sv_pass.slot;
        hipStream_t fs = r0.sv_pass.fs;
        if (n > 1) {
            // The unpack goes on shard 0's filter stream, in front of the frame's filter passes.  hazard (b): that stream runs the
            // filters frame after frame, so k_svgf_temporal of frame f - 2 -- the last reader of slot k -- is behind us in stream
            // order (and shard 0's path half of frame f + 2, the next writer of slot k, waits for r0.sv_ev_prepare[k], which the
            // filter half records behind this frame's k_svgf_temporal).  Shard 0's own path half writes other pixels of the planes.
            for (int i = 1; i < n; i++) ATN_HIP(hipStreamWaitEvent(fs, ev_sv_pushed[k][i], 0));
            r0.prof_begin(prof, ATN_K_SVGF_UNPACK, fs);
            hipLaunchKernelGGL(k_svgf_unpack_tiles, dim3(gl.unpack_grid), dim3(256), 0, fs, (const float4*)sv_gathered[k].p, r0.sv_contribs[k].p,
                               r0.sv_gnd[k].p, r0.sv_gam[k].p, r0.sv_primary[k].p, d->width, d->height, n, slots);
            r0.prof_end(prof);
            ATN_HIP(hipGetLastError());
            ATN_HIP(hipEventRecord(ev_sv_unpacked[k], fs));
            sv_unpacked_recorded[k] = true;
        }
        // hazard (c): the filter half waits for shard 0's path half itself (its bank's ev_gather, or stream order with one frame in
        // flight) and follows the unpack in stream order
        rc = r0.svgf_filter_half(d, out_host, stages_host);
        if (rc != ATN_OK) return fail(rc, "shard 0: " + r0.last_error);
        return ATN_OK;
    }

    int svgf_reset()
    {
        int rc = synchronize();
        if (rc) return rc;
        for (int i = 0; i < n; i++) (void)shard[i]->svgf_reset();
        sv_gw = 0; sv_gh = 0;       // (the next frame re-initialises every shard's planes and starts at slot 0 everywhere)
        sv_unpacked_recorded[0] = sv_unpacked_recorded[1] = false;
        return ATN_OK;
    }

    int synchronize()
    {
        int rc = on_all([&](int i) -> int {
            PathTracing& r = *shard[i];
            if (hipSetDevice(r.device) != hipSuccess) return r.fail(ATN_ERR_HIP, "hipSetDevice");
            return r.quiesce();
        });
        if (rc != ATN_OK) return rc;
        ATN_HIP(hipSetDevice(shard[0]->device));
        ATN_HIP(hipStreamSynchronize(comm));
        return ATN_OK;
    }
};

} // namespace atn
