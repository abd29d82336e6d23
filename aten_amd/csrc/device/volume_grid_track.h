// Dense-grid media: the box clip, the nearest-voxel lookup and the two tracking loops (HeterogeneousMedium::Sample and
// EvaluateTransmittance, src/libaten/volume/medium.cpp:58-202; GridUtil, volume/grid.cpp:12-43), written ONCE for the device
// (device/volume_grid.hpp) and for the CPU twin the tests hold it to (under tests/cxx): both include this file, so the expression order
// of every float operation is the same text.  Plain C++ over floats; the sampler and the tie marker are template arguments.
// docs/VOLUME.md ("Grid media") has the decisions: the flight ends at the surface, the transmittance walk ends at p2, the caps.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define ATN_VG_FN __host__ __device__ inline
#else
#define ATN_VG_FN inline
#endif

namespace atn_vg {

constexpr uint32_t kVolGridStepsMax = 16384u;       // steps after which either tracking loop stops (the reference loops while (true))
constexpr float kVolGridStepsBound = 1024.0F;       // majorant * box diagonal above this is refused: the expected steps across the grid

// One grid as the loops read it: x fastest, dim[0] * dim[1] * dim[2] floats.  hi = origin + dim * voxel_size, inv_voxel = 1 / voxel_size.
struct Grid {
    const float* density;
    int32_t dx, dy, dz;
    float ox, oy, oz;
    float inv_voxel;
    float hx, hy, hz;
};

ATN_VG_FN Grid make_grid(const float* density, const int32_t dim[3], const float origin[3], float voxel_size)
{
    Grid g;
    g.density = density;
    g.dx = dim[0]; g.dy = dim[1]; g.dz = dim[2];
    g.ox = origin[0]; g.oy = origin[1]; g.oz = origin[2];
    g.inv_voxel = 1.0F / voxel_size;
    g.hx = origin[0] + (float)dim[0] * voxel_size;
    g.hy = origin[1] + (float)dim[1] * voxel_size;
    g.hz = origin[2] + (float)dim[2] * voxel_size;
    return g;
}

// a tie marker that marks nothing (the device); the twin's records decisions within a relative 1e-5 of flipping
struct NoTie {
    ATN_VG_FN void cmp(float, float) {}
    ATN_VG_FN void face(float) {}
};

// one axis of the slab test.  false: the ray misses the slab
ATN_VG_FN bool clip_axis(float lo, float hi, float o, float d, float& t0, float& t1)
{
    if (d == 0.0F) return o >= lo && o < hi;
    const float a = (lo - o) / d;
    const float b = (hi - o) / d;
    if (!(a == a) || !(b == b)) return false;       // (fminf / fmaxf would drop a NaN operand and let the ray through)
    const float tn = fminf(a, b);
    const float tf = fmaxf(a, b);
    t0 = fmaxf(t0, tn);
    t1 = fminf(t1, tf);
    return true;
}

// GridUtil::ClipRayByGridBoundingBox: the ray org + t * dir, t in [0, t_end], against the grid's world box.  A slab test in float,
// x then y then z.  false (a miss, an empty interval, or a NaN in the ray: every slab distance is tested, and `t0 < t1` fails on a
// NaN t_end): the medium is not there for this ray and nothing is drawn.
ATN_VG_FN bool clip(const Grid& g, float ox, float oy, float oz, float dx, float dy, float dz, float t_end, float& t0, float& t1)
{
    t0 = 0.0F;
    t1 = t_end;
    if (!clip_axis(g.ox, g.hx, ox, dx, t0, t1)) return false;
    if (!clip_axis(g.oy, g.hy, oy, dy, t0, t1)) return false;
    if (!clip_axis(g.oz, g.hz, oz, dz, t0, t1)) return false;
    return t0 < t1;
}

// GetValueInGrid: worldToIndexF, Coord::Floor, the accessor's value (0 outside: NanoVDB's background)
template <class Tie>
ATN_VG_FN float density_at(const Grid& g, float px, float py, float pz, Tie& tie)
{
    const float fx = (px - g.ox) * g.inv_voxel;
    const float fy = (py - g.oy) * g.inv_voxel;
    const float fz = (pz - g.oz) * g.inv_voxel;
    tie.face(fx); tie.face(fy); tie.face(fz);
    const float ix = floorf(fx), iy = floorf(fy), iz = floorf(fz);
    if (!(ix >= 0.0F && ix < (float)g.dx && iy >= 0.0F && iy < (float)g.dy && iz >= 0.0F && iz < (float)g.dz)) return 0.0F;
    const uint32_t i = ((uint32_t)(int32_t)iz * (uint32_t)g.dy + (uint32_t)(int32_t)iy) * (uint32_t)g.dx + (uint32_t)(int32_t)ix;
    return g.density[i];
}

// -log(1 - u) / majorant with the logarithm in double, rounded once (as the homogeneous free flight, docs/VOLUME.md "Decisions")
ATN_VG_FN float step_length(float u, float majorant) { return -(float)log((double)(1.0F - u)) / majorant; }

enum { kFlightMiss = 0, kFlightEnd = 1, kFlightScatter = 2, kFlightCapped = 3 };

// HeterogeneousMedium::Sample.  The draws: u, then r, then on a scatter r_0, r_1 (left to the caller, who samples the phase function).
//   kFlightMiss     the clip missed: the ray stays where it is, nothing was drawn
//   kFlightEnd      the flight reached its end `s` = min(box exit, t_surface): the origin moves there, no event
//   kFlightScatter  a scatter at `s`; `factor` = tr * (sigma_s_at / prob_sigma_s) / pdf multiplies the throughput
//   kFlightCapped   kVolGridStepsMax steps: counted by the caller, then as kFlightEnd
// An absorption (sigma_a_at * le / prob_sigma_a; the reference goes on tracking behind it) multiplies `le_factor`, 1 otherwise:
// sigma_a != 0 is refused on the device, the branch is kept as written.
template <class Smp, class Tie>
ATN_VG_FN int delta_track(const Grid& g, float sigma_a, float sigma_s, float majorant, float ox, float oy, float oz, float dx, float dy, float dz,
                          float t_surface, Smp& smp, Tie& tie, float& s, uint32_t& steps, float& factor, float& le_factor)
{
    float min_s, max_s;
    steps = 0u; factor = 1.0F; le_factor = 1.0F; s = 0.0F;
    if (!clip(g, ox, oy, oz, dx, dy, dz, t_surface, min_s, max_s)) return kFlightMiss;
    float sample_s = min_s;
    while (steps < kVolGridStepsMax) {
        const float u = smp.next();
        const float ds = step_length(u, majorant);
        sample_s += ds;
        steps++;
        tie.cmp(sample_s, max_s);
        if (sample_s >= max_s) { s = max_s; return kFlightEnd; }
        const float density = density_at(g, ox + dx * sample_s, oy + dy * sample_s, oz + dz * sample_s, tie);
        const float sigma_a_at = sigma_a * density;
        const float sigma_s_at = sigma_s * density;
        const float prob_sigma_a = sigma_a_at / majorant;
        const float prob_sigma_s = sigma_s_at / majorant;
        int mode = 0;       // TrackMode: 0 Null, 1 Absorption, 2 Scattering
        const float r = smp.next();
        tie.cmp(r, prob_sigma_s);
        if (prob_sigma_s < prob_sigma_a) {
            if (r < prob_sigma_s) mode = 2;
            else if (r < prob_sigma_a) mode = 1;
        }
        else {
            if (r < prob_sigma_a) mode = 1;
            else if (r < prob_sigma_s) mode = 2;
        }
        if (mode == 0) continue;
        const float tr = (float)exp((double)(-majorant * ds));      // HomogeniousMedium::EvaluateTransmittance(majorant, ds)
        const float pdf = majorant * tr;
        if (mode == 1) le_factor = le_factor * (tr * (sigma_a_at / prob_sigma_a) / pdf);
        else {
            factor = tr * (sigma_s_at / prob_sigma_s) / pdf;
            s = sample_s;
            return kFlightScatter;
        }
    }
    s = max_s;
    return kFlightCapped;
}

// HeterogeneousMedium::EvaluateTransmittance along org + t * dir, t in [0, distance] (the walk ends at p2, docs/VOLUME.md).
// Returns the transmittance; `capped`: kVolGridStepsMax steps were taken (the caller counts the connection as blocked).
// As written, a collision both survives with probability sigma_n / majorant and is weighted by it.
template <class Smp, class Tie>
ATN_VG_FN float ratio_track(const Grid& g, float sigma_a, float sigma_s, float majorant, float ox, float oy, float oz, float dx, float dy, float dz,
                            float distance, Smp& smp, Tie& tie, uint32_t& steps, bool& capped)
{
    float min_s, max_s;
    capped = false;
    if (!clip(g, ox, oy, oz, dx, dy, dz, distance, min_s, max_s)) return 1.0F;
    float sample_s = min_s;
    float transmittance = 1.0F;
    uint32_t n = 0u;
    while (n < kVolGridStepsMax) {
        const float u = smp.next();
        const float ds = step_length(u, majorant);
        sample_s += ds;
        n++;
        tie.cmp(sample_s, max_s);
        if (sample_s > max_s) { steps += n; return transmittance; }
        const float density = density_at(g, ox + dx * sample_s, oy + dy * sample_s, oz + dz * sample_s, tie);
        const float sigma_a_at = sigma_a * density;
        const float sigma_s_at = sigma_s * density;
        const float sigma_n = majorant - sigma_a_at - sigma_s_at;
        const float r = smp.next();
        tie.cmp(r, sigma_n / majorant);
        if (r >= sigma_n / majorant) { steps += n; return 0.0F; }
        transmittance *= (sigma_n / majorant);
    }
    steps += n;
    capped = true;
    return transmittance;
}

} // namespace atn_vg
