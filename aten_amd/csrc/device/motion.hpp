// Geometry motion vectors (docs/MOTION.md): the motion pass of SVGF and ReSTIR for geometry that moves.  It stands in for the reference's
// G-buffer raster pass over moving geometry (drawSceneForGBuffer: a previous position per vertex, a previous local-to-world matrix
// per object), from what a frame already has in device memory:
//   k_motion_capture_ids  per slot, behind the bounce-0 trace: the primary hit record -> the frame's ids plane
//                         {objid (int bits; -1 = miss), triangle id (int bits), a, b}, indexed by pixel
//   k_motion_geometry     per pixel: ids -> object record -> the triangle's indices -> its three vertices and the instance's matrix as
//                         the GEOMETRY HISTORY holds them (the scene the last frame of this kind saw) -> previous world position;
//                         with the frame's own bounce-0 position, motion_depth's arithmetic (svgf_frame.hpp) on the two
//   k_motion_copy         a range of the scene's vertex positions / matrices -> the history (what a tick wrote, and only that)
// Per pixel the motion kernel makes three dependent 16-byte gathers (object -> triangle -> three vertices + four matrix rows); neighbouring
// pixels mostly share the triangle, so a wave's gathers fall into a few cache lines.  No LDS.
#pragma once
#include "kernels.hpp"
#include "svgf_frame.hpp"

namespace atn {

struct MotionArgs {
    const float4* ids;                  // the frame's ids plane (k_motion_capture_ids)
    const float4* pos;                  // the frame's bounce-0 world positions, xyz (SVGF: primary_position; ReSTIR: info[2])
    const atn_object_param* objects;    // of the scene set the frame reads
    const atn_triangle_param* tris;
    const float4* h_vtx;                // the history: vertex positions ...
    const float4* h_mtx;                // ... and matrices, 4 rows per mat4
    float4* motion;                     // motion.xy, clip w, 1 -- what k_svgf_temporal / ReSTIR's temporal reuse read
    float w2c[16], prev_w2c[16];
    int32_t width, height;
    uint32_t n_objects, n_tris, n_vtx, h_mtx_quads;     // sizes of the arrays above: a record that points outside them is a miss
};

// aten_amd.hip fills MotionArgs and calls the launchers (launch.hpp); the kernels are compiled in motion.hip only
#ifdef ATN_MOTION_TU

__global__ void __launch_bounds__(256) k_motion_capture_ids(PathBuffers pb, FrameParams fp, float4* ids)
{
    const uint32_t slot = (uint32_t)fp.slot_begin + blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= (uint32_t)fp.slot_end) return;
    int32_t x, y;
    if (!slot_to_pixel(fp, slot, x, y)) return;
    const float4 is4 = pb.isect[slot];      // {objid, a, b, tri}
    const bool hit = __float_as_int(is4.x) >= 0;
    ids[y * fp.width + x] = hit ? make_float4(is4.x, is4.w, is4.y, is4.z) : make_float4(__int_as_float(-1), __int_as_float(-1), 0.0F, 0.0F);
}

__global__ void __launch_bounds__(256) k_motion_geometry(MotionArgs g)
{
    SvgfFrame sf;       // (only the frame's size: svgf_pixel's block -> tile map, the filter passes' tile shape)
    sf.width = g.width; sf.height = g.height;
    int32_t ix, iy;
    if (!svgf_pixel(sf, ix, iy)) return;
    const int32_t idx = ix + iy * g.width;
    const float4 id4 = g.ids[idx];
    const int32_t objid = __float_as_int(id4.x), tri_id = __float_as_int(id4.y);
    float4 md = make_float4(0.0F, 0.0F, -1.0F, 1.0F);
    if (objid >= 0 && (uint32_t)objid < g.n_objects && (uint32_t)tri_id < g.n_tris) {
        // evaluate_hit's object lookup (shading.hpp): {type, area, object_id, mtx_id} is the record's first 16 bytes
        const float4 o4 = reinterpret_cast<const float4*>(&g.objects[objid])[0];
        const bool is_inst = __float_as_int(o4.x) == ATN_OBJ_INSTANCE;
        const int32_t mtx_id = is_inst ? __float_as_int(o4.w) : -1;
        const float4 t4 = reinterpret_cast<const float4*>(&g.tris[tri_id])[0];      // idx[3], pad
        const uint32_t i0 = __float_as_uint(t4.x), i1 = __float_as_uint(t4.y), i2 = __float_as_uint(t4.z);
        if (i0 < g.n_vtx && i1 < g.n_vtx && i2 < g.n_vtx && (mtx_id < 0 || 4u * (uint32_t)mtx_id + 3u < g.h_mtx_quads)) {
            const float4 p0 = g.h_vtx[i0], p1 = g.h_vtx[i1], p2 = g.h_vtx[i2];
            m4 L2W = m4_identity();
            if (mtx_id >= 0) {
                L2W.r0 = g.h_mtx[4 * mtx_id + 0]; L2W.r1 = g.h_mtx[4 * mtx_id + 1];
                L2W.r2 = g.h_mtx[4 * mtx_id + 2]; L2W.r3 = g.h_mtx[4 * mtx_id + 3];
            }
            // evaluate_hit's position, operation by operation, over the history's vertices and matrix
            const float a = id4.z, b = id4.w;
            const float c = 1 - a - b;
            const float4 P = add4(add4(mul4(c, p0), mul4(a, p1)), mul4(b, p2));
            const f3 pp = m4_apply(L2W, mk3(P));
            const float4 wp = g.pos[idx];
            // motion_depth's arithmetic (svgf_frame.hpp): the current clip position from the frame's own position, the previous one
            // from the history's
            const float* m = g.w2c;
            const float* n = g.prev_w2c;
            const float cx = m[0] * wp.x + m[1] * wp.y + m[2] * wp.z + m[3] * 1.0F;
            const float cy = m[4] * wp.x + m[5] * wp.y + m[6] * wp.z + m[7] * 1.0F;
            const float cw = m[12] * wp.x + m[13] * wp.y + m[14] * wp.z + m[15] * 1.0F;
            const float px = n[0] * pp.x + n[1] * pp.y + n[2] * pp.z + n[3] * 1.0F;
            const float py = n[4] * pp.x + n[5] * pp.y + n[6] * pp.z + n[7] * 1.0F;
            const float pw = n[12] * pp.x + n[13] * pp.y + n[14] * pp.z + n[15] * 1.0F;
            const float csx = (cx / cw) * 0.5F + 0.5F, csy = (cy / cw) * 0.5F + 0.5F;
            const float psx = (px / pw) * 0.5F + 0.5F, psy = (py / pw) * 0.5F + 0.5F;
            md = make_float4(psx - csx, psy - csy, cw, 1.0F);
        }
    }
    g.motion[idx] = md;
}

// dst[i] = src[i] for n float4s (the caller passes both pointers at the range's first element)
__global__ void __launch_bounds__(256) k_motion_copy(float4* __restrict__ dst, const float4* __restrict__ src, uint32_t n)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

#endif  // ATN_MOTION_TU

} // namespace atn
