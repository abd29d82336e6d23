// CPU twin of the geometry motion pass (aten_amd/csrc/device/motion.hpp: k_motion_geometry): docs/MOTION.md's semantics as a function of
// the ids plane, the objects, the triangles, the current and the history's vertices and matrices, and the two camera matrices.  It
// restates this repository's own kernel arithmetic -- evaluate_hit's position (csrc/device/shading.hpp) and motion_depth
// (csrc/device/svgf_frame.hpp) -- with one IEEE fp32 rounding per operation (compiled with -ffp-contract=off -fno-fast-math).
// TEST INFRASTRUCTURE ONLY: compiled by tests/motion_oracle.py; the product never sees it.
#include <cstdint>
#include <cstring>

namespace {

struct V4 { float x, y, z, w; };
struct Obj { int32_t type; float area; int32_t object_id, mtx_id, triangle_id, triangle_num, light_id, pad0; float sphere[4]; int32_t sphere_mtrl, pad1[3]; };
static_assert(sizeof(Obj) == 64, "atn_object_param");
struct Tri { int32_t idx[3]; float pad; float area; int32_t need_normal, mtrlid, mesh_id; };
static_assert(sizeof(Tri) == 32, "atn_triangle_param");

V4 mul4(float s, const V4& v) { return V4{ s * v.x, s * v.y, s * v.z, s * v.w }; }
V4 add4(const V4& a, const V4& b) { return V4{ a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w }; }

// c p0 + a p1 + b p2 in that order, then the local-to-world matrix (rows r[0..3] of a row-major mat4; null = the identity matrix,
// applied like any other)
V4 world_position(const Tri& t, const V4* vtx, const float* m, float a, float b)
{
    static const float ident[16] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1 };
    if (!m) m = ident;
    const V4 p0 = vtx[t.idx[0]], p1 = vtx[t.idx[1]], p2 = vtx[t.idx[2]];
    const float c = 1 - a - b;
    const V4 P = add4(add4(mul4(c, p0), mul4(a, p1)), mul4(b, p2));
    V4 r;
    r.x = ((m[0] * P.x + m[1] * P.y) + m[2] * P.z) + m[3];
    r.y = ((m[4] * P.x + m[5] * P.y) + m[6] * P.z) + m[7];
    r.z = ((m[8] * P.x + m[9] * P.y) + m[10] * P.z) + m[11];
    r.w = 1.0f;
    return r;
}

} // namespace

extern "C" {

// ids: {objid bits, tri bits, a, b} per pixel.  instance_type: ATN_OBJ_INSTANCE.  An instance with mtx_id >= 0 uses matrix mtx_id of
// cur_mtx / h_mtx (mat4s, row-major); anything else the identity.  out_motion: {prev - cur in screen fractions, current clip w, 1},
// (0, 0, -1, 1) on a miss; out_pos (may be null): the current world position, w = 1 (zeros on a miss).
void orc_motion_geometry(const V4* ids, uint32_t n, const Obj* objects, int32_t instance_type, const Tri* tris, const V4* cur_vtx, const V4* h_vtx,
                         const float* cur_mtx, const float* h_mtx, const float* w2c, const float* prev_w2c, V4* out_motion, V4* out_pos)
{
    for (uint32_t i = 0; i < n; i++) {
        int32_t objid, tri;
        std::memcpy(&objid, &ids[i].x, 4); std::memcpy(&tri, &ids[i].y, 4);
        V4 md{ 0.0f, 0.0f, -1.0f, 1.0f };
        V4 wp{ 0.0f, 0.0f, 0.0f, 0.0f };
        if (objid >= 0) {
            const Obj& o = objects[objid];
            const int32_t mtx_id = o.type == instance_type ? o.mtx_id : -1;
            const float a = ids[i].z, b = ids[i].w;
            wp = world_position(tris[tri], cur_vtx, mtx_id >= 0 ? cur_mtx + 16 * (size_t)mtx_id : nullptr, a, b);
            const V4 pp = world_position(tris[tri], h_vtx, mtx_id >= 0 ? h_mtx + 16 * (size_t)mtx_id : nullptr, a, b);
            const float* m = w2c;
            const float* q = prev_w2c;
            const float cx = m[0] * wp.x + m[1] * wp.y + m[2] * wp.z + m[3] * 1.0f;
            const float cy = m[4] * wp.x + m[5] * wp.y + m[6] * wp.z + m[7] * 1.0f;
            const float cw = m[12] * wp.x + m[13] * wp.y + m[14] * wp.z + m[15] * 1.0f;
            const float px = q[0] * pp.x + q[1] * pp.y + q[2] * pp.z + q[3] * 1.0f;
            const float py = q[4] * pp.x + q[5] * pp.y + q[6] * pp.z + q[7] * 1.0f;
            const float pw = q[12] * pp.x + q[13] * pp.y + q[14] * pp.z + q[15] * 1.0f;
            const float csx = (cx / cw) * 0.5f + 0.5f, csy = (cy / cw) * 0.5f + 0.5f;
            const float psx = (px / pw) * 0.5f + 0.5f, psy = (py / pw) * 0.5f + 0.5f;
            md = V4{ psx - csx, psy - csy, cw, 1.0f };
        }
        out_motion[i] = md;
        if (out_pos) out_pos[i] = wp;
    }
}

// the static pass (motion_depth): one world position through both cameras; w = 0 is a miss
void orc_motion_static(const V4* pos, uint32_t n, const float* w2c, const float* prev_w2c, V4* out_motion)
{
    for (uint32_t i = 0; i < n; i++) {
        const V4 wp = pos[i];
        V4 md{ 0.0f, 0.0f, -1.0f, 1.0f };
        if (wp.w != 0.0f) {
            const float* m = w2c;
            const float* q = prev_w2c;
            const float cx = m[0] * wp.x + m[1] * wp.y + m[2] * wp.z + m[3] * 1.0f;
            const float cy = m[4] * wp.x + m[5] * wp.y + m[6] * wp.z + m[7] * 1.0f;
            const float cw = m[12] * wp.x + m[13] * wp.y + m[14] * wp.z + m[15] * 1.0f;
            const float px = q[0] * wp.x + q[1] * wp.y + q[2] * wp.z + q[3] * 1.0f;
            const float py = q[4] * wp.x + q[5] * wp.y + q[6] * wp.z + q[7] * 1.0f;
            const float pw = q[12] * wp.x + q[13] * wp.y + q[14] * wp.z + q[15] * 1.0f;
            const float csx = (cx / cw) * 0.5f + 0.5f, csy = (cy / cw) * 0.5f + 0.5f;
            const float psx = (px / pw) * 0.5f + 0.5f, psy = (py / pw) * 0.5f + 0.5f;
            md = V4{ psx - csx, psy - csy, cw, 1.0f };
        }
        out_motion[i] = md;
    }
}

uint32_t orc_motion_sizeof_object(void) { return (uint32_t)sizeof(Obj); }

} // extern "C"
