/*
 * VOLUME GRID ORACLE -- TEST INFRASTRUCTURE ONLY (tests/volume_grid_oracle.py compiles it; the product never loads it).
 *
 * tests/cxx/volume_oracle.cpp with the grid branches added: a medium whose grid_idx names one of the grids handed in is heterogeneous
 * (HeterogeneousMedium::Sample / EvaluateTransmittance, src/libaten/volume/medium.cpp:58-202; SampleMedium, TraverseRayInMedium,
 * volume_pathtracing_impl.h:79-224).  The clip, the voxel lookup and both tracking loops are the product's own header,
 * aten_amd/csrc/device/volume_grid_track.h, included here: one text for both sides.  With the decisions of docs/VOLUME.md ("Grid
 * media"): the flight ends at the surface, the transmittance walk ends at p2, a connection draws from a stream of its own, both loops
 * stop after kVolGridStepsMax steps.  On a scene without grid media every output equals volume_oracle.cpp's byte for byte.
 *
 * A CPU restatement of the reference's volume path tracer for homogeneous media -- aten::VolumePathTracing::OnRender, radiance and
 * Nee (src/libaten/renderer/volume/volume_pathtracing.cpp:22-89,228-407,436-533), UpdateMedium, SampleMedium, TraverseRayInMedium
 * and TraverseShadowRay (volume_pathtracing_impl.h:24-294), HomogeniousMedium (volume/medium.h:26-122) and the Henyey-Greenstein
 * phase function (volume/phase_function.h) -- on top of the path-tracing oracle (oracle/orc_pt.h, read as it is), with the decisions
 * of docs/VOLUME.md: a push onto a full medium stack is dropped and counted, a connection that has crossed 64 boundaries counts as
 * blocked and is counted.
 */
#include "../../oracle/orc_pt.h"
#include "../../include/aten_amd.h"
#include "../../aten_amd/csrc/device/volume_grid_track.h"
#include <omp.h>
#include <cmath>
#include <cstring>
#include <vector>

using namespace orc;

namespace {

constexpr int kStack = 8;           // MedisumStackSize, pt_params.h:22 -- also the cap on radiance's loop
constexpr int kWalkMax = 64;        // boundaries a connection may cross (docs/VOLUME.md)
constexpr int32_t kVolume = 15;     // MaterialType::Volume

struct Medium { float g, sigma_a, sigma_s; int32_t grid_idx; float majorant; float le[3]; };
static_assert(sizeof(Medium) == sizeof(atn_medium_param), "MediumParameter");
Medium medium_of(const atn_material_param& m) { Medium r; std::memcpy(&r, m.medium, sizeof(r)); return r; }

// aten::stack<int32_t, 8> (misc/stack.h): top() is queue_.front(), the FIRST medium entered, not the last
struct MStack {
    int32_t q[kStack]; int32_t n{ 0 };
    MStack() { for (int i = 0; i < kStack; i++) q[i] = 0; }
    bool empty() const { return n == 0; }
    int32_t top() const { return q[0]; }
    bool push(int32_t id) { if (n >= kStack) return false; q[n++] = id; return true; }
    void pop() { n -= 1; }
};

struct Counters { uint64_t stack_overflow{ 0 }, walk_overflow{ 0 }, connections{ 0 }, segments{ 0 }, flight_capped{ 0 }, conn_capped{ 0 }; };

// ---- the grids of a render (set by the entry points before any thread starts, read only afterwards) ------------------------------
struct GridSet { std::vector<atn_vg::Grid> grids; bool in_use{ false }; };
const GridSet* g_grids = nullptr;
const atn_vg::Grid* grid_of(const struct Medium& m);

// the sampler as the tracking loops draw from it
struct Draw {
    CMJ& s;
    float next() { return s.nextSample(); }
};
// marks a decision that lay within a relative 1e-5 of flipping: sample_s against the flight's end, r against a probability, an index
// coordinate against a voxel face
struct Tie {
    bool near{ false };
    void cmp(float a, float b) { if (std::fabs(a - b) <= 1e-5F * std::fmax(std::fabs(a), std::fabs(b))) near = true; }
    void face(float f) { if (std::fabs(f - std::round(f)) <= 1e-5F * std::fmax(1.0F, std::fabs(f))) near = true; }
};
// the connection's own stream: Cmj{idx, dim at the moment the record is written, scramble ^ 0x5bd1e995}
CMJ connection_stream(const CMJ& path) { CMJ c; c.init(path.m_idx, path.m_dimension, path.m_scramble ^ 0x5bd1e995u); return c; }

// ---- volume/phase_function.h ----------------------------------------------------------------------------------------------------
float HG_Evaluate(float g, const v3& wi, const v3& wo)
{
    g = clamp_(g, -1.0F, 1.0F);
    const float g2 = sqr(g);
    const float costheta = dot(wi, wo);
    const float _4pi = 4 * PI;
    return (1 - g2) / (_4pi * std::pow(1 + g2 - 2 * g * costheta, 1.5F));
}
v3 HG_SampleDirection(float r1, float r2, float g, const v3& w)
{
    g = clamp_(g, -1.0F, 1.0F);
    float costheta = 0.0F;
    if (std::fabs(g) < EPS) costheta = 1 - 2 * r1;
    else {
        const float g2 = sqr(g);
        costheta = 1 / (2 * g) * (1 + g2 - sqr((1 - g2) / (1 - g + 2 * g * r1)));
    }
    const float sintheta = std::sqrt(1 - costheta * costheta);
    const float phi = PI_2 * r2;
    const float cosphi = std::cos(phi);
    const float sinphi = std::sin(phi);
    v3 t, b;
    GetTangentCoordinate(w, t, b);
    v3 dir = t * sintheta * cosphi + b * sintheta * sinphi + w * costheta;
    dir = normalize(dir);
    return dir;
}

// ---- volume/medium.h:26-122 -----------------------------------------------------------------------------------------------------
float sigma_t_of(const Medium& m) { return m.sigma_a + m.sigma_s; }
// kind: 0 no event, 1 absorbed, 2 scattered
bool HomogeniousMedium_Sample(v3& throughput, CMJ& sampler, const Ray& curr_ray, const Medium& medium, float distance_to_surface,
                              Ray& next_ray, float* s_out, int32_t* kind)
{
    const float sigma_a = medium.sigma_a;
    const float sigma_t = sigma_t_of(medium);
    const float r1 = sampler.nextSample();
    const float s = -std::log(fmax_(1.0F - r1, 0.0F)) / sigma_t;
    if (s_out) *s_out = s;
    if (s >= distance_to_surface) {
        next_ray = curr_ray;
        next_ray.org += next_ray.dir * distance_to_surface;
        if (kind) *kind = 0;
        return false;
    }
    const float r2 = sampler.nextSample();
    const float Pa = sigma_a / sigma_t;
    next_ray = curr_ray;
    next_ray.org += next_ray.dir * s;
    if (r2 < Pa) {
        throughput *= v3(medium.le[0], medium.le[1], medium.le[2]);
        if (kind) *kind = 1;
    }
    else {
        const float r3 = sampler.nextSample();
        const float r4 = sampler.nextSample();
        next_ray.dir = HG_SampleDirection(r3, r4, medium.g, -curr_ray.dir);
        next_ray.dir = normalize(next_ray.dir);
        if (kind) *kind = 2;
    }
    return true;
}

const atn_vg::Grid* grid_of(const Medium& m)
{
    if (!g_grids || m.grid_idx < 0 || (size_t)m.grid_idx >= g_grids->grids.size()) return nullptr;
    return &g_grids->grids[(size_t)m.grid_idx];
}

// HeterogeneousMedium::Sample, medium.cpp:58-151, with the flight ending at min(box exit, distance_to_surface)
bool HeterogeneousMedium_Sample(v3& throughput, CMJ& sampler, const Ray& curr_ray, const Medium& medium, const atn_vg::Grid& grid, float distance_to_surface,
                                Ray& next_ray, float* s_out, int32_t* kind, uint32_t* steps_out, bool* tie_out, bool* clipped, Counters* cnt)
{
    Draw draw{ sampler };
    Tie tie;
    float s = 0.0F, factor = 1.0F, le_factor = 1.0F;
    uint32_t steps = 0;
    const int ev = atn_vg::delta_track(grid, medium.sigma_a, medium.sigma_s, medium.majorant, curr_ray.org.x, curr_ray.org.y, curr_ray.org.z,
                                       curr_ray.dir.x, curr_ray.dir.y, curr_ray.dir.z, distance_to_surface, draw, tie, s, steps, factor, le_factor);
    if (s_out) *s_out = s;
    if (steps_out) *steps_out = steps;
    if (tie_out) *tie_out = tie.near;
    if (clipped) *clipped = ev != atn_vg::kFlightMiss;
    if (kind) *kind = ev == atn_vg::kFlightScatter ? 2 : 0;
    if (ev == atn_vg::kFlightCapped && cnt) cnt->flight_capped++;
    next_ray = curr_ray;
    if (le_factor != 1.0F) throughput *= v3(medium.le[0], medium.le[1], medium.le[2]) * le_factor;
    if (ev == atn_vg::kFlightMiss) return false;
    next_ray.org += next_ray.dir * s;
    if (ev != atn_vg::kFlightScatter) return false;
    const float r_0 = sampler.nextSample();
    const float r_1 = sampler.nextSample();
    next_ray.dir = HG_SampleDirection(r_0, r_1, medium.g, -curr_ray.dir);
    next_ray.dir = normalize(next_ray.dir);
    throughput *= v3(factor);
    return true;
}

// ---- volume_pathtracing_impl.h --------------------------------------------------------------------------------------------------
void UpdateMedium(const Ray& ray, const v3& wo, const v3& surface_normal, const atn_material_param& mtrl, MStack& st, Counters* cnt)
{
    const v3 wi = -ray.dir;
    const bool is_trasmitted = (dot(wo, surface_normal) < 0) != (dot(wi, surface_normal) < 0);
    const bool is_enter = dot(wi, surface_normal) > 0;
    if (is_trasmitted) {
        if (is_enter) {
            if (mtrl.is_medium) { if (!st.push(mtrl.id) && cnt) cnt->stack_overflow++; }
        }
        else if (st.n > 0) st.pop();
    }
}
bool IsSubsurface(const atn_material_param& m) { return m.type != kVolume && m.is_medium; }
Medium CurrentMedium(const Scene& ctxt, const MStack& st) { return medium_of(ctxt.GetMaterial((uint32_t)st.top())); }

struct WalkOut { float transmittance{ 1.0F }; int32_t segments{ 0 }; v3 org, dir; float t_max{ 0 }; uint32_t track_steps{ 0 }, stream_dim{ 0 }; bool tie{ false }; };

// the transmittance of the segment org .. org + distance * dir in `medium`.  false: the tracking loop hit its cap
bool Segment(const Medium& medium, const v3& org, const v3& dir, float distance, CMJ& conn, WalkOut& wo, float& transmittance, Counters* cnt)
{
    if (const atn_vg::Grid* grid = grid_of(medium)) {
        Draw draw{ conn };
        Tie tie;
        bool capped = false;
        const float tr = atn_vg::ratio_track(*grid, medium.sigma_a, medium.sigma_s, medium.majorant, org.x, org.y, org.z, dir.x, dir.y, dir.z, distance,
                                             draw, tie, wo.track_steps, capped);
        wo.stream_dim = conn.m_dimension;
        if (tie.near) wo.tie = true;
        transmittance *= tr;
        if (capped && cnt) cnt->conn_capped++;
        return !capped;
    }
    transmittance *= std::exp(-sigma_t_of(medium) * distance);
    return true;
}

bool TraverseRayInMedium(const Scene& ctxt, const LightSampleResult& ls, const v3& start_point, const v3& surface_nml, MStack st,
                         WalkOut& wo, Counters* cnt, CMJ conn)
{
    float transmittance = 1.0F;
    v3 nml = dot(ls.dir, surface_nml) > 0 ? surface_nml : -surface_nml;
    Ray ray(start_point, ls.dir, nml);
    float distance_to_light = ls.dist_to_light;
    if (ls.attrib & ATN_LIGHT_ATTR_INFINITE) distance_to_light = length(ls.pos - start_point);
    float t_max = distance_to_light - ctxt.cfg().epsilon_bias_for_traversing_shadow_ray_in_medium;
    wo.org = ray.org; wo.dir = ray.dir; wo.t_max = t_max;
    wo.stream_dim = conn.m_dimension;
    if (cnt) cnt->connections++;
    int32_t crossed = 0;
    while (true) {
        Isect isect;
        if (cnt) cnt->segments++;
        wo.segments++;
        const bool is_hit = TraverseClosest(isect, ctxt, ray, EPS, t_max, nullptr);
        if (is_hit) {
            HitRec hrec;
            evaluate_hit_result(hrec, ctxt.GetObject((uint32_t)isect.objid), ctxt, ray, isect);
            atn_material_param mtrl;
            FillMaterial(mtrl, ctxt, hrec.mtrlid);
            const bool is_enter = dot(-ray.dir, hrec.normal) > 0;
            // volume_pathtracing_impl.h:152-160 blocks on `!is_medium || is_enter`, which makes every pure medium boundary met from
            // outside an occluder; here only a surface with an interior blocks when entered (docs/VOLUME.md)
            if (!mtrl.is_medium || (is_enter && IsSubsurface(mtrl))) { wo.transmittance = transmittance; return false; }
            if (crossed >= kWalkMax) { if (cnt) cnt->walk_overflow++; wo.transmittance = transmittance; return false; }
            crossed++;
            if (!st.empty() && !Segment(CurrentMedium(ctxt, st), ray.org, ray.dir, length(ray.org - hrec.p), conn, wo, transmittance, cnt)) {
                wo.transmittance = transmittance;
                return false;
            }
            UpdateMedium(ray, ray.dir, hrec.normal, mtrl, st, cnt);
            nml = dot(ray.dir, hrec.normal) > 0 ? hrec.normal : -hrec.normal;
            ray = Ray(hrec.p, ray.dir, nml);
            t_max -= isect.t;
        }
        else {
            if (!st.empty()) {
                const v3 end_p = ray.org + t_max * ray.dir;
                if (!Segment(CurrentMedium(ctxt, st), ray.org, ray.dir, length(ray.org - end_p), conn, wo, transmittance, cnt)) {
                    wo.transmittance = transmittance;
                    return false;
                }
            }
            break;
        }
    }
    wo.transmittance = transmittance;
    return true;
}

struct VState {
    MStack st; int32_t depth_count{ 0 }; bool will_update_depth{ false };
    bool sh_active{ false }; v3 sh_org, sh_dir;     // aten::ShadowRay: isActive survives an iteration that ends before Nee clears it
};

// what one iteration of radiance leaves behind (the stage buffers of atn_volume_download)
struct IterRec {
    uint32_t flags{ 0 };        // 1 processed, 2 hit, 4 medium sampled, 8 absorbed, 16 scattered, 32 passed through, 64 connection, 128 visible, 256 terminated
    float s{ 0 }, hit_t{ 0 };
    int32_t depth_count{ 0 }, stack_n{ 0 }; int32_t stack[kStack]{};
    uint32_t dim{ 0 };
    v3 ray_org, ray_dir;
    WalkOut walk;
    uint32_t flight_steps{ 0 };
    bool flight_tie{ false };
};
enum { R_PROCESSED = 1, R_HIT = 2, R_SAMPLED = 4, R_ABSORBED = 8, R_SCATTERED = 16, R_PASSED = 32, R_CONN = 64, R_VISIBLE = 128, R_TERMINATED = 256 };

bool SampleLight(const Scene& ctxt, const atn_material_param& mtrl, CMJ& sampler, const v3& org, const v3& nml, bool is_on_surface,
                 LightSampleResult& ls, float& select_prob)
{
    const int32_t lightnum = ctxt.GetLightNum();
    const bool is_invalid_mtrl = is_on_surface && (attr_singular(mtrl) || attr_translucent(mtrl));
    if (lightnum <= 0 || is_invalid_mtrl) return false;
    const int32_t target = std::min<int32_t>(static_cast<int32_t>(sampler.nextSample() * lightnum), lightnum - 1);
    select_prob = 1.0f / lightnum;
    Light_sample(ls, ctxt.GetLight(target), ctxt, org, nml, &sampler);
    return true;
}

// VolumePathTracing::Nee, volume_pathtracing.cpp:228-407
void Nee(PathState& path, VState& vs, const Scene& ctxt, Ray& ray_io, const Isect& isect, int32_t rrDepth, IterRec& rec_out, Counters* cnt)
{
    const int32_t bounce = vs.depth_count;
    const float russianProb = ComputeRussianProbability(bounce, rrDepth, path);
    if (path.is_terminated) { vs.will_update_depth = false; return; }
    path.throughput /= russianProb;

    Ray ray = ray_io;
    HitRec rec;
    evaluate_hit_result(rec, ctxt.GetObject((uint32_t)isect.objid), ctxt, ray, isect);
    const bool isBackfacing = dot(rec.normal, -ray.dir) < 0.0F;
    v3 orienting_normal = rec.normal;
    atn_material_param mtrl;
    FillMaterial(mtrl, ctxt, rec.mtrlid);

    vs.sh_active = false;
    bool is_scattered = false;
    if (!vs.st.empty()) {
        Ray next_ray;
        int32_t kind = 0;
        const Medium medium = CurrentMedium(ctxt, vs.st);
        if (const atn_vg::Grid* grid = grid_of(medium)) {
            bool clipped = false;
            is_scattered = HeterogeneousMedium_Sample(path.throughput, path.sampler, ray, medium, *grid, isect.t, next_ray, &rec_out.s, &kind,
                                                      &rec_out.flight_steps, &rec_out.flight_tie, &clipped, cnt);
            rec_out.flags |= (clipped ? R_SAMPLED : 0u) | (kind == 2 ? R_SCATTERED : 0u);
        }
        else {
            is_scattered = HomogeniousMedium_Sample(path.throughput, path.sampler, ray, medium, isect.t, next_ray, &rec_out.s, &kind);
            rec_out.flags |= R_SAMPLED | (kind == 1 ? R_ABSORBED : 0u) | (kind == 2 ? R_SCATTERED : 0u);
        }
        if (is_scattered) { vs.sh_active = true; vs.sh_org = next_ray.org; vs.sh_dir = next_ray.dir; }
        ray = next_ray;
    }
    bool is_reflected_or_refracted = false;
    if (is_scattered) ray_io = ray;
    else {
        if (HitImplicitLight(ctxt, isect.objid, isBackfacing, bounce, path, ray, rec, mtrl)) { vs.will_update_depth = false; return; }
        const Ray curr_ray = ray;
        if (mtrl.is_medium && !IsSubsurface(mtrl)) {
            const v3 ray_base_nml = dot(ray.dir, orienting_normal) > 0 ? orienting_normal : -orienting_normal;
            ray_io = Ray(rec.p, ray.dir, ray_base_nml);
            rec_out.flags |= R_PASSED;
        }
        else {
            const v4 albedo = sampleTexture(ctxt, mtrl.albedoMap, rec.u, rec.v, v4(mtrl.baseColor.x, mtrl.baseColor.y, mtrl.baseColor.z, mtrl.baseColor.w));
            if (!attr_translucent(mtrl) && isBackfacing) orienting_normal = -orienting_normal;
            float pre_sampled_r;
            { v3 nn; pre_sampled_r = applyNormal(ctxt, mtrl, orienting_normal, nn, rec.u, rec.v, ray.dir, &path.sampler); orienting_normal = nn; }
            LightSampleResult ls; float select_prob = 0.0F;
            if (SampleLight(ctxt, mtrl, path.sampler, rec.p, orienting_normal, true, ls, select_prob)) {
                rec_out.flags |= R_CONN;
                const bool visible = TraverseRayInMedium(ctxt, ls, rec.p, orienting_normal, vs.st, rec_out.walk, cnt, connection_stream(path.sampler));
                if (visible) {
                    rec_out.flags |= R_VISIBLE;
                    v3 radiance;
                    if (ComputeRadianceNEE(radiance, ctxt, ray.dir, orienting_normal, mtrl, rec.u, rec.v, select_prob, ls, pre_sampled_r))
                        path.contrib += path.throughput * rec_out.walk.transmittance * radiance * albedo.xyz();
                }
            }
            MaterialSampling sampling;
            sampleMaterial(&sampling, ctxt, &mtrl, orienting_normal, ray.dir, &path.sampler, rec.u, rec.v, pre_sampled_r);
            Ray out = ray_io;
            PrepareForNextBounce(rec, russianProb, orienting_normal, mtrl, sampling, albedo.xyz(), path, out);
            ray_io = out;
            is_reflected_or_refracted = true;
        }
        UpdateMedium(curr_ray, ray_io.dir, orienting_normal, mtrl, vs.st, cnt);
    }
    vs.will_update_depth = is_scattered || is_reflected_or_refracted;
}

// TraverseShadowRay, volume_pathtracing_impl.h:231-294
void TraverseShadowRay(PathState& path, VState& vs, const Scene& ctxt, const Isect& isect, int32_t max_depth, IterRec& rec_out, Counters* cnt)
{
    if (vs.sh_active) {
        const v3 org = vs.sh_org, nml = vs.sh_dir;
        atn_material_param mtrl;
        FillMaterial(mtrl, ctxt, isect.mtrlid);
        LightSampleResult ls; float select_prob = 0.0F;
        if (SampleLight(ctxt, mtrl, path.sampler, org, nml, false, ls, select_prob)) {
            rec_out.flags |= R_CONN;
            rec_out.walk = WalkOut();
            const bool visible = TraverseRayInMedium(ctxt, ls, org, nml, vs.st, rec_out.walk, cnt, connection_stream(path.sampler));
            if (visible) {
                rec_out.flags |= R_VISIBLE;
                const Medium medium = CurrentMedium(ctxt, vs.st);
                const float phase_f = HG_Evaluate(medium.g, -nml, ls.dir);
                const float dist2 = sqr(ls.dist_to_light);
                const float G = 1.0F / dist2;
                const v3 Ls = rec_out.walk.transmittance * phase_f * G * ls.light_color / ls.pdf / select_prob;
                path.contrib += path.throughput * Ls;
            }
        }
    }
    if (vs.will_update_depth) vs.depth_count += 1;
    vs.will_update_depth = false;
    if (vs.depth_count > max_depth) path.is_terminated = true;
}

// VolumePathTracing::radiance, volume_pathtracing.cpp:22-89.  log: kStack records, one per iteration (null = none)
void Radiance(PathState& path, VState& vs, Ray& ray, int32_t ix, int32_t iy, int32_t w, int32_t h, const Scene& ctxt, const atn_camera_param& cam,
              int32_t maxDepth, int32_t rrDepth, IterRec* log, Counters* cnt)
{
    int32_t loop_count = 0;
    while (!path.is_terminated) {
        if (loop_count >= kStack) { path.is_terminated = true; if (log) log[kStack - 1].flags |= R_TERMINATED; break; }
        IterRec r;
        r.flags = R_PROCESSED;
        path.isHit = false;
        Isect isect;
        if (TraverseClosest(isect, ctxt, ray, EPS, INF, nullptr)) {
            path.isHit = true;
            r.flags |= R_HIT; r.hit_t = isect.t;
            Nee(path, vs, ctxt, ray, isect, rrDepth, r, cnt);
            TraverseShadowRay(path, vs, ctxt, isect, maxDepth, r, cnt);
        }
        else {
            ShadeMiss(ix, iy, w, h, vs.depth_count, ctxt, cam, path, ray);
            path.is_terminated = true;
        }
        if (log) {
            if (path.is_terminated) r.flags |= R_TERMINATED;
            r.depth_count = vs.depth_count; r.stack_n = vs.st.n;
            for (int k = 0; k < kStack; k++) r.stack[k] = k < vs.st.n ? vs.st.q[k] : 0;
            r.dim = path.sampler.m_dimension; r.ray_org = ray.org; r.ray_dir = ray.dir;
            log[loop_count] = r;
        }
        loop_count++;
    }
}

void write_rec(const IterRec& r, uint32_t* state, uint32_t* stack, atn_vec4* rayb, atn_vec4* conn, uint32_t* ties = nullptr)
{
    const bool grid = g_grids && g_grids->in_use;       // (the GRID kernels run: the flight's steps and the connection's stream are kept)
    if (ties) *ties = (r.flight_tie ? 1u : 0u) | (r.walk.tie && (r.flags & R_CONN) ? 2u : 0u);
    if (state) { state[0] = r.flags | (grid ? r.flight_steps << 16 : 0u); state[1] = (uint32_t)r.depth_count; state[2] = (uint32_t)r.stack_n; state[3] = r.dim; }
    if (stack) for (int k = 0; k < 4; k++) stack[k] = ((uint32_t)r.stack[2 * k] & 0xffffu) | (((uint32_t)r.stack[2 * k + 1] & 0xffffu) << 16);
    if (rayb) { rayb[0] = atn_vec4{ r.ray_org.x, r.ray_org.y, r.ray_org.z, r.s }; rayb[1] = atn_vec4{ r.ray_dir.x, r.ray_dir.y, r.ray_dir.z, r.hit_t }; }
    if (conn) {
        const bool c = (r.flags & R_CONN) != 0;
        conn[0] = c ? atn_vec4{ r.walk.org.x, r.walk.org.y, r.walk.org.z, r.walk.t_max } : atn_vec4{ 0, 0, 0, 0 };
        conn[1] = c ? atn_vec4{ r.walk.dir.x, r.walk.dir.y, r.walk.dir.z, r.walk.transmittance } : atn_vec4{ 0, 0, 0, 0 };
        conn[2] = c ? atn_vec4{ (float)r.walk.segments, (r.flags & R_VISIBLE) ? 1.0F : 0.0F, grid ? (float)r.walk.track_steps : 0.0F,
                                grid ? (float)r.walk.stream_dim : 0.0F } : atn_vec4{ 0, 0, 0, 0 };
    }
}

} // namespace

extern "C" {

struct orc_destination {    // oracle/aten_oracle.cpp's
    int32_t width, height, maxDepth, russianRouletteDepth, sample;
    uint32_t frame;
    int32_t progressive;
    int32_t nthreads;
};

// One frame into `film` (vec4[w*h], progressive or overwrite as orc_render).  break_on_terminate: a terminated path ends the pixel's
// sample loop (volume_pathtracing.cpp:518-520; every path that leaves radiance is terminated).  Stage buffers of sample 0 after
// iteration `capture` (< 0: none; null = skip): state uint32[n][4] {flags, depth_count, stack size, CMJ dimension}, stack uint32[n][4]
// (eight 16-bit ids), ray vec4[n][2] {next org, s} {next dir, hit t}, conn vec4[n][3] {org, t_max} {dir, transmittance} {segments,
// visible, 0, 0}; counters uint64[6] {stack overflow, walk overflow, connections, segments, grid flights capped, grid connections
// capped}.  grids[n_grids]: atn_volume_set_grids' (the densities are read in place).  When a medium names one of them: the flight's
// step count sits in bits 16-30 of the flags, conn[2] = {segments, visible, ratio-tracking steps, final dimension of the
// connection's stream}, and ties uint32[n] (null = skip) marks the captured iteration's near ties: 1 the flight, 2 the connection.
int orc_vol_render(const atn_scene_desc* scene, const atn_camera_param* camera, const uint32_t* seeds, uint32_t n_seeds,
                   const orc_destination* dst, int32_t break_on_terminate, atn_vec4* film, int32_t capture,
                   uint32_t* state, uint32_t* stack, atn_vec4* rayb, atn_vec4* conn, uint64_t* counters,
                   const atn_volume_grid* grids, uint32_t n_grids, uint32_t* ties)
{
    Scene ctxt(scene);
    GridSet gs;
    for (uint32_t i = 0; i < n_grids; i++) gs.grids.push_back(atn_vg::make_grid(grids[i].density, grids[i].dim, grids[i].origin, grids[i].voxel_size));
    for (uint32_t i = 0; i < scene->n_materials; i++) {
        const atn_material_param& m = scene->materials[i];
        if (m.is_medium && medium_of(m).grid_idx >= 0 && (uint32_t)medium_of(m).grid_idx < n_grids) gs.in_use = true;
    }
    g_grids = &gs;
    const int32_t width = dst->width, height = dst->height;
    int32_t maxDepth = dst->maxDepth;
    int32_t rrDepth = dst->russianRouletteDepth;
    if (rrDepth > maxDepth) rrDepth = maxDepth - 1;
    if (dst->nthreads > 0) omp_set_num_threads(dst->nthreads);
    const uint32_t samples = (uint32_t)dst->sample;
    Counters total;
#pragma omp parallel
    {
        Counters local;
#pragma omp for schedule(dynamic, 4)
        for (int32_t y = 0; y < height; y++) {
            for (int32_t x = 0; x < width; x++) {
                const int32_t idx = y * width + x;
                v3 col(0); uint32_t cnt = 0;
                PathState path; path.samples = 0;
                IterRec log[kStack];
                for (uint32_t i = 0; i < samples; i++) {
                    Ray ray;
                    GeneratePath(ray, x, y, (int32_t)i, dst->frame, path, *camera, seeds[idx % n_seeds]);
                    path.contrib = v3(0);
                    VState vs;      // PathThroughput::medium is cleared with the path
                    Radiance(path, vs, ray, x, y, width, height, ctxt, *camera, maxDepth, rrDepth, (i == 0 && capture >= 0) ? log : nullptr, &local);
                    if (isInvalidColor(path.contrib)) continue;
                    col += path.contrib;
                    cnt++;
                    if (break_on_terminate && path.is_terminated) break;
                }
                col /= (float)cnt;
                const v4 v(col, 1);
                atn_vec4& cur = film[idx];
                if (dst->progressive) {
                    const float nn = static_cast<float>(static_cast<int32_t>(cur.w));
                    v4 cc(cur.x, cur.y, cur.z, cur.w);
                    cc = nn * cc + v;
                    const float d = nn + 1;
                    cur.x = cc.x / d; cur.y = cc.y / d; cur.z = cc.z / d;
                    cur.w = nn + 1;
                }
                else { cur.x = v.x; cur.y = v.y; cur.z = v.z; cur.w = v.w; }
                if (capture >= 0 && capture < kStack)
                    write_rec(log[capture], state ? state + 4 * (size_t)idx : nullptr, stack ? stack + 4 * (size_t)idx : nullptr,
                              rayb ? rayb + 2 * (size_t)idx : nullptr, conn ? conn + 3 * (size_t)idx : nullptr, ties ? ties + idx : nullptr);
            }
        }
#pragma omp critical
        {
            total.stack_overflow += local.stack_overflow; total.walk_overflow += local.walk_overflow; total.connections += local.connections; total.segments += local.segments;
            total.flight_capped += local.flight_capped; total.conn_capped += local.conn_capped;
        }
    }
    if (counters) {
        counters[0] = total.stack_overflow; counters[1] = total.walk_overflow; counters[2] = total.connections; counters[3] = total.segments;
        counters[4] = total.flight_capped; counters[5] = total.conn_capped;
    }
    g_grids = nullptr;
    return 0;
}

// ---- the two tracking loops as plain functions, along org + t * dir ----
// a sampler that keeps what it handed out, and a tie marker that keeps every sample_s and index coordinate it was shown
struct LogDraw {
    CMJ& s; float* out; uint32_t cap; uint32_t n{ 0 };
    float next() { const float v = s.nextSample(); if (out && n < cap) out[n] = v; n++; return v; }
};
struct LogTie : Tie {
    float* s_out; float* idx_out; uint32_t cap; uint32_t ns{ 0 }, ni{ 0 }; bool first{ true };
    LogTie(float* s, float* i, uint32_t c) : s_out(s), idx_out(i), cap(c) {}
    void cmp(float a, float b) { Tie::cmp(a, b); first = !first; if (!first && s_out && ns < cap) s_out[ns] = a; if (!first) ns++; }
    void face(float f) { Tie::face(f); if (idx_out && ni < 3 * cap) idx_out[ni] = f; ni++; }
};
// HeterogeneousMedium::Sample for n streams (index i % 256, dimension dim0, scramble[i]) over [0, t_surface]: kind[i] 0 miss, 1 end,
// 2 scatter, 3 capped; s[i]; steps[i]; draws[i] the stream's dimension afterwards (the scatter's r_0, r_1 are not drawn here);
// factor[i]; tie[i].  With log_cap > 0 stream 0 is logged: log_draws[2 log_cap] what it drew, log_s[log_cap] sample_s of each step,
// log_idx[3 log_cap] the index coordinates of each lookup.
void orc_volg_delta_track(const atn_volume_grid* grid, float sigma_a, float sigma_s, float majorant, const float* org, const float* dir, float t_surface,
                          uint32_t n, uint32_t dim0, const uint32_t* scramble, int32_t* kind, float* s, uint32_t* steps, uint32_t* draws, float* factor, uint32_t* tie,
                          uint32_t log_cap, float* log_draws, float* log_s, float* log_idx)
{
    const atn_vg::Grid g = atn_vg::make_grid(grid->density, grid->dim, grid->origin, grid->voxel_size);
    for (uint32_t i = 0; i < n; i++) {
        CMJ smp; smp.init(i % 256u, dim0, scramble[i]);
        float le_factor = 1.0F;
        if (i == 0 && log_cap) {
            LogDraw draw{ smp, log_draws, 2 * log_cap };
            LogTie t(log_s, log_idx, log_cap);
            kind[i] = atn_vg::delta_track(g, sigma_a, sigma_s, majorant, org[0], org[1], org[2], dir[0], dir[1], dir[2], t_surface, draw, t, s[i], steps[i], factor[i], le_factor);
            tie[i] = t.near ? 1u : 0u;
        }
        else {
            Draw draw{ smp };
            Tie t;
            kind[i] = atn_vg::delta_track(g, sigma_a, sigma_s, majorant, org[0], org[1], org[2], dir[0], dir[1], dir[2], t_surface, draw, t, s[i], steps[i], factor[i], le_factor);
            tie[i] = t.near ? 1u : 0u;
        }
        draws[i] = smp.m_dimension;
    }
}
// HeterogeneousMedium::EvaluateTransmittance for n connection streams (index i % 256, dimension dim0, scramble[i] ^ 0x5bd1e995) over [0, distance]: tr[i], steps[i], capped[i]
void orc_volg_ratio_track(const atn_volume_grid* grid, float sigma_a, float sigma_s, float majorant, const float* org, const float* dir, float distance,
                          uint32_t n, uint32_t dim0, const uint32_t* scramble, float* tr, uint32_t* steps, uint32_t* capped)
{
    const atn_vg::Grid g = atn_vg::make_grid(grid->density, grid->dim, grid->origin, grid->voxel_size);
    for (uint32_t i = 0; i < n; i++) {
        CMJ smp; smp.init(i % 256u, dim0, scramble[i] ^ 0x5bd1e995u);
        Draw draw{ smp };
        Tie t;
        bool cap = false;
        steps[i] = 0;
        tr[i] = atn_vg::ratio_track(g, sigma_a, sigma_s, majorant, org[0], org[1], org[2], dir[0], dir[1], dir[2], distance, draw, t, steps[i], cap);
        capped[i] = cap ? 1u : 0u;
    }
}

// One path by hand: the ray (org, dir) with the sampler of GeneratePath(frame, rnd) behind its two camera draws, through radiance.
// Per iteration (8 records): state[4], stack[4], ray[2], conn[3] as orc_vol_render.  Returns the iterations run; contrib: vec3.
int32_t orc_vol_trace_path(const atn_scene_desc* scene, const atn_camera_param* camera, const float* org, const float* dir, uint32_t frame, uint32_t rnd,
                           int32_t maxDepth, int32_t rrDepth, uint32_t* state, uint32_t* stack, atn_vec4* rayb, atn_vec4* conn, float* contrib)
{
    Scene ctxt(scene);
    PathState path; path.samples = 0;
    Ray ray;
    GeneratePath(ray, 0, 0, 0, frame, path, *camera, rnd);
    ray = Ray(v3(org[0], org[1], org[2]), v3(dir[0], dir[1], dir[2]));
    path.contrib = v3(0);
    VState vs;
    IterRec log[kStack];
    Counters c;
    Radiance(path, vs, ray, 0, 0, camera->width, camera->height, ctxt, *camera, maxDepth, rrDepth, log, &c);
    int32_t n = 0;
    for (int k = 0; k < kStack; k++) {
        if (log[k].flags & R_PROCESSED) n = k + 1;
        write_rec(log[k], state + 4 * k, stack + 4 * k, rayb + 2 * k, conn + 3 * k);
    }
    contrib[0] = path.contrib.x; contrib[1] = path.contrib.y; contrib[2] = path.contrib.z;
    return n;
}

// TraverseRayInMedium from `start` (normal `nml`) towards light `light_idx`, with the medium stack `ids[n_ids]`:
// out = {visible, transmittance, segments, walk overflow}
void orc_vol_connect(const atn_scene_desc* scene, const float* start, const float* nml, int32_t light_idx, const int32_t* ids, int32_t n_ids, float* out)
{
    Scene ctxt(scene);
    CMJ smp; smp.init(0, 0, 0);
    const v3 p(start[0], start[1], start[2]), n(nml[0], nml[1], nml[2]);
    LightSampleResult ls;
    Light_sample(ls, ctxt.GetLight((uint32_t)light_idx), ctxt, p, n, &smp);
    MStack st;
    for (int32_t i = 0; i < n_ids; i++) st.push(ids[i]);
    WalkOut wo; Counters c;
    const bool vis = TraverseRayInMedium(ctxt, ls, p, n, st, wo, &c, connection_stream(smp));
    out[0] = vis ? 1.0F : 0.0F; out[1] = wo.transmittance; out[2] = (float)wo.segments; out[3] = (float)c.walk_overflow;
}

// ---- the phase function and the free-flight sampler as plain functions ----
void orc_vol_phase_eval(float g, uint32_t n, const float* wi, const float* wo, float* out)
{
    for (uint32_t i = 0; i < n; i++) out[i] = HG_Evaluate(g, v3(wi[3 * i], wi[3 * i + 1], wi[3 * i + 2]), v3(wo[3 * i], wo[3 * i + 1], wo[3 * i + 2]));
}
void orc_vol_phase_sample(float g, uint32_t n, const float* w, const float* r1, const float* r2, float* out)
{
    for (uint32_t i = 0; i < n; i++) {
        const v3 d = HG_SampleDirection(r1[i], r2[i], g, v3(w[3 * i], w[3 * i + 1], w[3 * i + 2]));
        out[3 * i] = d.x; out[3 * i + 1] = d.y; out[3 * i + 2] = d.z;
    }
}
// HomogeniousMedium::Sample for n samplers (index i % 256, dimension 0, scramble[i]) along +z from the origin over `distance`:
// kind[i] 0 / 1 / 2, s[i], draws[i], thr[3 i] the throughput after (1 before), dir[3 i] the next direction
void orc_vol_medium_sample(const float* medium8, float distance, uint32_t n, const uint32_t* scramble, int32_t* kind, float* s, int32_t* draws,
                           float* thr, float* dir)
{
    Medium m; std::memcpy(&m, medium8, sizeof(m));
    for (uint32_t i = 0; i < n; i++) {
        CMJ smp; smp.init(i % 256u, 0, scramble[i]);
        v3 t(1.0F);
        const Ray r(v3(0, 0, 0), v3(0, 0, 1));
        Ray next;
        HomogeniousMedium_Sample(t, smp, r, m, distance, next, &s[i], &kind[i]);
        draws[i] = (int32_t)smp.m_dimension;
        thr[3 * i] = t.x; thr[3 * i + 1] = t.y; thr[3 * i + 2] = t.z;
        dir[3 * i] = next.dir.x; dir[3 * i + 1] = next.dir.y; dir[3 * i + 2] = next.dir.z;
    }
}
uint32_t orc_vol_sizeof_medium() { return (uint32_t)sizeof(atn_medium_param); }

} // extern "C"
