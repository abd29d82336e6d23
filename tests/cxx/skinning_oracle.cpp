// CPU twin of the device skinning (aten_amd/csrc/device/skinning.hpp): the expressions of the reference's skinning kernels, evaluated
// with libaten's HOST definitions, one IEEE fp32 rounding per operation (compiled with -ffp-contract=off -fno-fast-math).
// TEST INFRASTRUCTURE ONLY: compiled by tests/skinning_oracle.py; the product never sees it.
//
//   computeSkinning    src/libidaten/kernel/Skinning.cu:8-54
//   setTriangleParam   src/libidaten/kernel/Skinning.cu:56-82
//   getMinMax          src/libidaten/kernel/Skinning.cu:89-145
#include <cmath>
#include <cstdint>
#include <cstring>

namespace {

struct V4 { float x, y, z, w; };
struct M4 { float m[4][4]; };          // row-major, applied as M * p (math/mat4.h:10-25)
struct SkinVtx {                       // aten::SkinningVertex, deformable/SkinningVertex.h:7-14
    float position[4];
    float normal[3];
    uint8_t clr[4];
    float uv[2];
    float blend_index[4];
    float blend_weight[4];
};
static_assert(sizeof(SkinVtx) == 72, "SkinningVertex");
struct Tri { int32_t idx[3]; float pad; float area; int32_t need_normal, mtrlid, mesh_id; };     // aten::TriangleParameter
static_assert(sizeof(Tri) == 32, "TriangleParameter");

// float * mat4: a copy, then mat4::operator*=(float) -- 16 products m *= t (math/mat4.h:157-164, 603-608)
M4 scale(float t, const M4& m)
{
    M4 r = m;
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) r.m[i][j] *= t;
    return r;
}
// mat4 * vec4 = mat4::apply(vec4): the four sums in the order written (math/mat4.h:171-180, 597-601)
V4 apply(const M4& m, const V4& p)
{
    V4 r;
    r.x = m.m[0][0] * p.x + m.m[0][1] * p.y + m.m[0][2] * p.z + m.m[0][3] * p.w;
    r.y = m.m[1][0] * p.x + m.m[1][1] * p.y + m.m[1][2] * p.z + m.m[1][3] * p.w;
    r.z = m.m[2][0] * p.x + m.m[2][1] * p.y + m.m[2][2] * p.z + m.m[2][3] * p.w;
    r.w = m.m[3][0] * p.x + m.m[3][1] * p.y + m.m[3][2] * p.z + m.m[3][3] * p.w;
    return r;
}
// vec4::operator+= (math/vec4.h:150-157)
void add(V4& a, const V4& b) { a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w; }
// normalize(vec4) = v * rsqrt(dot(v, v)), host rsqrt = 1 / sqrt (math/vec4.h:271-275, 288-293; math/math.h:33-40)
V4 normalize(const V4& v)
{
    const float d = v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
    const float inv = 1.0F / std::sqrt(d);
    return V4{ inv * v.x, inv * v.y, inv * v.z, inv * v.w };
}

// the box's order: the floats' order with -0 below +0 and a NaN above every number (skinning.hpp, skin_key), so that the
// result does not depend on the order of the reduction; for every other input aten::min / aten::max (math/math.h:128-176)
uint32_t key(float f)
{
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
float unkey(uint32_t k)
{
    const uint32_t u = (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k;
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}

} // namespace

extern "C" {

uint32_t orc_skin_sizeof_vertex() { return (uint32_t)sizeof(SkinVtx); }

// One Skinning::compute.  pos / nml / prev hold the previous tick's values on entry (pos is read when !restart); tris are the skin's
// triangles with indices RELATIVE to the skin's first vertex (idx - vtx_offset of the scene's); box = min xyz, max xyz.
void orc_skin_compute(const SkinVtx* vtx, uint32_t n_vtx, const M4* mtx, int32_t restart, V4* pos, V4* nml, V4* prev,
                      Tri* tris, uint32_t n_tris, float* box)
{
    uint32_t kmin[3] = { 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu }, kmax[3] = { 0u, 0u, 0u };
    for (uint32_t i = 0; i < n_vtx; i++) {
        const SkinVtx& v = vtx[i];
        const V4 p{ v.position[0], v.position[1], v.position[2], v.position[3] };
        const V4 n{ v.normal[0], v.normal[1], v.normal[2], 0.0F };                 // Skinning.cu:25
        V4 rp{ 0, 0, 0, 0 }, rn{ 0, 0, 0, 0 };
        for (int b = 0; b < 4; b++) {                                               // Skinning.cu:31-39
            const int32_t idx = (int32_t)v.blend_index[b];
            const M4 m = scale(v.blend_weight[b], mtx[idx]);
            add(rp, apply(m, p));
            add(rn, apply(m, n));
        }
        rn = normalize(rn);                                                         // Skinning.cu:41
        if (restart) prev[i] = V4{ rp.x, rp.y, rp.z, 1.0F };                        // Skinning.cu:43-50
        else { prev[i] = pos[i]; prev[i].w = 1.0F; }
        pos[i] = V4{ rp.x, rp.y, rp.z, v.uv[0] };                                   // Skinning.cu:52-53
        nml[i] = V4{ rn.x, rn.y, rn.z, v.uv[1] };
        const float c[3] = { rp.x, rp.y, rp.z };
        for (int k = 0; k < 3; k++) {
            const uint32_t kk = key(c[k]);
            if (kk < kmin[k]) kmin[k] = kk;
            if (kk > kmax[k]) kmax[k] = kk;
        }
    }
    for (uint32_t t = 0; t < n_tris; t++) {                                         // Skinning.cu:68-77
        const V4 &v0 = pos[tris[t].idx[0]], &v1 = pos[tris[t].idx[1]], &v2 = pos[tris[t].idx[2]];
        const V4 a{ v1.x - v0.x, v1.y - v0.y, v1.z - v0.z, v1.w - v0.w }, b{ v2.x - v0.x, v2.y - v0.y, v2.z - v0.z, v2.w - v0.w };
        const V4 c{ a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x, 0.0F };     // math/vec4.h:277-286
        tris[t].area = std::sqrt(c.x * c.x + c.y * c.y + c.z * c.z);                // vec4::length, math/vec4.h:199-203: not halved
    }
    for (int k = 0; k < 3; k++) { box[k] = unkey(kmin[k]); box[3 + k] = unkey(kmax[k]); }
}

} // extern "C"
