// Skinning on the device: the first step of the deformation tick (idaten::Skinning::compute, src/libidaten/kernel/Skinning.cu:227-345;
// computeSkinning :8-54, setTriangleParam :56-82, getMinMax :89-145).  docs/SKINNING.md has the decisions.
//
// The arithmetic is the reference's, evaluated with libaten's HOST definitions (one IEEE rounding per operation, no contraction):
//   weight * mtx        mat4::operator*=(float): 16 products                                  (math/mat4.h:157-164, 603-608)
//   (.) * vec4          mat4::apply: per row ((x + y) + z) + w                                 (math/mat4.h:171-180)
//   result += (.)       componentwise, bones 0 .. 3 in order, from vec4(0)                     (math/vec4.h:150-157)
//   normalize(vec4)     v * (1 / sqrt(dot4(v, v)))                                             (math/vec4.h:271-293, math/math.h:33-40)
//   area                length(cross(v1 - v0, v2 - v0)) over xyz, not halved                   (math/vec4.h:199-203, 277-286)
// so the results equal those of a host build of the same expressions bit for bit (the tests keep one, docs/SKINNING.md).
//
// A skinned mesh has 10^3 .. 10^5 vertices at 136 B each: a few microseconds of HBM time, less than one kernel boundary.  What a tick
// costs is its launches, so there are two (the reference: four and a blocking read-back):
//   k_skin_vertices    one thread per vertex: the block's 72-byte records through LDS (one contiguous 18 KB run, read as 8-byte words --
//                      not 18 strided dwords per lane), the palette from LDS when it fits, positions / normals / previous positions
//                      out, and the block's box: wave64 shuffles, one LDS step, six words per block
//   k_skin_triangles   one thread per triangle: the area into the scene's triangle, the triangle's shading record (what
//                      k_pack_shade_tris writes, kernels.hpp) -- and block 0 folds the blocks' boxes into the skin's box
// The box is reduced on an order-preserving integer image of the floats (skin_key), so it does not depend on the order of the
// reduction: -0 sorts below +0 (the minimum of {-0, +0} is -0, the maximum +0), a NaN above every number.  For every other input it
// is aten::min / aten::max over the positions.
#pragma once
#include "scene_dev.hpp"

namespace atn {

constexpr uint32_t kSkinBlock = 256;
constexpr uint32_t kSkinVtxWords = 9;           // a SkinningVertex is nine 8-byte words
constexpr uint32_t kSkinPaletteLds = 256;       // matrices (16 KB): larger palettes are read from global memory
constexpr uint32_t kSkinMaxMatrices = 65536;

struct SkinVtxArgs {
    const uint2* verts;         // atn_skinning_vertex[n_vtx]
    const float4* palette;      // 4 rows per matrix
    float4* pos; float4* nml;   // the scene's arrays at the skin's first vertex
    float4* prev;               // the skin's own
    uint32_t* partial;          // [blocks][6] keys: min xyz, max xyz
    uint32_t n_vtx, n_mtx;
    int32_t restart;
};
struct SkinTriArgs {
    atn_triangle_param* tris;   // the scene's arrays (triangles hold scene-wide vertex indices)
    const float4* vtx_pos; const float4* vtx_nml;
    float4* shade_tris;
    uint32_t first, count;
    const uint32_t* partial; uint32_t n_partial;
    float* box;                 // min xyz, max xyz
};

#ifdef ATN_SKINNING_TU    // (the kernels: skinning.hip; aten_amd.hip reads the declarations above)

ATN_DEV uint32_t skin_key(float f)
{
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
ATN_DEV float skin_unkey(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

// min of k[0..2], max of k[3..5] over the block; the result is valid in thread 0 .. 5 (component = thread)
ATN_DEV uint32_t skin_block_reduce(uint32_t (&k)[6], uint32_t* s_red)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            k[c] = min(k[c], (uint32_t)__shfl_xor((int)k[c], off));
            k[c + 3] = max(k[c + 3], (uint32_t)__shfl_xor((int)k[c + 3], off));
        }
    }
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < 6; c++) s_red[wave * 6u + (uint32_t)c] = k[c];
    }
    __syncthreads();
    uint32_t r = 0;
    if (threadIdx.x < 6u) {
        r = s_red[threadIdx.x];
#pragma unroll
        for (uint32_t w = 1; w < kSkinBlock / 64u; w++) {
            const uint32_t o = s_red[w * 6u + threadIdx.x];
            r = threadIdx.x < 3u ? min(r, o) : max(r, o);
        }
    }
    return r;
}

// (weight * mtx) * v, mat4::operator*=(float) then mat4::apply: the row's four products with the weight first
ATN_DEV float skin_row(const float4& m, float w, const float4& v)
{
    return (((m.x * w) * v.x + (m.y * w) * v.y) + (m.z * w) * v.z) + (m.w * w) * v.w;
}

template <bool PAL_LDS>
__global__ __launch_bounds__(kSkinBlock) void k_skin_vertices(SkinVtxArgs a)
{
    __shared__ uint2 s_vtx[kSkinBlock * kSkinVtxWords];
    __shared__ float4 s_pal[PAL_LDS ? 4u * kSkinPaletteLds : 1u];
    __shared__ uint32_t s_red[6u * (kSkinBlock / 64u)];
    const uint32_t tid = threadIdx.x, base = blockIdx.x * kSkinBlock;
    const uint32_t cnt = min(kSkinBlock, a.n_vtx - base), words = cnt * kSkinVtxWords;
    const uint2* g = a.verts + (size_t)base * kSkinVtxWords;
#pragma unroll
    for (uint32_t k = 0; k < kSkinVtxWords; k++) {
        const uint32_t j = k * kSkinBlock + tid;
        if (j < words) s_vtx[j] = g[j];
    }
    if (PAL_LDS)
        for (uint32_t j = tid; j < 4u * a.n_mtx; j += kSkinBlock) s_pal[j] = a.palette[j];
    __syncthreads();

    uint32_t key[6] = { 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u, 0u };
    if (tid < cnt) {
        uint2 r[kSkinVtxWords];
#pragma unroll
        for (uint32_t k = 0; k < kSkinVtxWords; k++) r[k] = s_vtx[tid * kSkinVtxWords + k];
        // position[4] | normal[3] clr | uv[2] | blend_index[4] | blend_weight[4]
        const float4 p = make_float4(__uint_as_float(r[0].x), __uint_as_float(r[0].y), __uint_as_float(r[1].x), __uint_as_float(r[1].y));
        const float4 n = make_float4(__uint_as_float(r[2].x), __uint_as_float(r[2].y), __uint_as_float(r[3].x), 0.0F);
        const float uv0 = __uint_as_float(r[4].x), uv1 = __uint_as_float(r[4].y);
        const float bi[4] = { __uint_as_float(r[5].x), __uint_as_float(r[5].y), __uint_as_float(r[6].x), __uint_as_float(r[6].y) };
        const float bw[4] = { __uint_as_float(r[7].x), __uint_as_float(r[7].y), __uint_as_float(r[8].x), __uint_as_float(r[8].y) };
        float4 rp = make_float4(0.0F, 0.0F, 0.0F, 0.0F), rn = rp;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint32_t m = (uint32_t)(int32_t)bi[i];        // in [0, n_mtx): atn_skin_create refused every other vertex
            const float4* row = (PAL_LDS ? (const float4*)s_pal : a.palette) + 4u * m;
            const float4 m0 = row[0], m1 = row[1], m2 = row[2], m3 = row[3];
            const float w = bw[i];
            rp.x = rp.x + skin_row(m0, w, p); rp.y = rp.y + skin_row(m1, w, p); rp.z = rp.z + skin_row(m2, w, p);
            rn.x = rn.x + skin_row(m0, w, n); rn.y = rn.y + skin_row(m1, w, n); rn.z = rn.z + skin_row(m2, w, n);
            rn.w = rn.w + skin_row(m3, w, n);
        }
        const float inv = 1.0F / sqrtf(((rn.x * rn.x + rn.y * rn.y) + rn.z * rn.z) + rn.w * rn.w);
        const uint32_t v = base + tid;
        if (a.restart) a.prev[v] = make_float4(rp.x, rp.y, rp.z, 1.0F);
        else { const float4 o = a.pos[v]; a.prev[v] = make_float4(o.x, o.y, o.z, 1.0F); }
        a.pos[v] = make_float4(rp.x, rp.y, rp.z, uv0);
        a.nml[v] = make_float4(inv * rn.x, inv * rn.y, inv * rn.z, uv1);
        key[0] = key[3] = skin_key(rp.x); key[1] = key[4] = skin_key(rp.y); key[2] = key[5] = skin_key(rp.z);
    }
    const uint32_t r = skin_block_reduce(key, s_red);
    if (tid < 6u) a.partial[blockIdx.x * 6u + tid] = r;
}

__global__ __launch_bounds__(kSkinBlock) void k_skin_triangles(SkinTriArgs a)
{
    __shared__ uint32_t s_red[6u * (kSkinBlock / 64u)];
    const uint32_t i = blockIdx.x * kSkinBlock + threadIdx.x;
    if (i < a.count) {
        const uint32_t t = a.first + i;
        float4* tp = reinterpret_cast<float4*>(&a.tris[t]);
        const float4 h0 = tp[0];
        float4 h1 = tp[1];
        const int32_t i0 = __float_as_int(h0.x), i1 = __float_as_int(h0.y), i2 = __float_as_int(h0.z);
        const float4 p0 = a.vtx_pos[i0], p1 = a.vtx_pos[i1], p2 = a.vtx_pos[i2];
        const float4 c = cross4(sub4(p1, p0), sub4(p2, p0));
        h1.x = sqrtf((c.x * c.x + c.y * c.y) + c.z * c.z);      // TriangleParameter::area
        tp[1] = h1;
        float4* q = a.shade_tris + (size_t)kShadeTriQuads * t;  // k_pack_shade_tris' record
        q[0] = p0; q[1] = p1; q[2] = p2;
        q[3] = a.vtx_nml[i0]; q[4] = a.vtx_nml[i1]; q[5] = a.vtx_nml[i2];
        q[6] = h1;
        q[7] = make_float4(h0.x, h0.y, h0.z, 0.0F);
    }
    if (blockIdx.x == 0) {
        uint32_t key[6] = { 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u, 0u };
        for (uint32_t b = threadIdx.x; b < a.n_partial; b += kSkinBlock) {
#pragma unroll
            for (int c = 0; c < 3; c++) {
                key[c] = min(key[c], a.partial[b * 6u + (uint32_t)c]);
                key[c + 3] = max(key[c + 3], a.partial[b * 6u + 3u + (uint32_t)c]);
            }
        }
        const uint32_t r = skin_block_reduce(key, s_red);
        if (threadIdx.x < 6u) a.box[threadIdx.x] = skin_unkey(r);
    }
}

// k_lbvh_morton (lbvh.hpp) with the normalisation box read from device memory: the skin's box never visits the host
__global__ __launch_bounds__(256) void k_lbvh_morton_box(const atn_triangle_param* __restrict__ tris, const float4* __restrict__ vtx,
                                                         int32_t vtx_offset, uint32_t n, const float* __restrict__ box,
                                                         uint32_t* __restrict__ codes, uint32_t* __restrict__ indices)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const f3 bmin = mk3(box[0], box[1], box[2]), bmax = mk3(box[3], box[4], box[5]);
    f3 mn, mx;
    lbvh_triangle_box(tris, vtx, vtx_offset, i, mn, mx);
    const f3 size = bmax - bmin;                    // aabb::size
    f3 c = (mn + mx) * 0.5F;
    c = (c - bmin) / size;
    codes[i] = lbvh_expand_bits(lbvh_quantise(c.x)) << 2 | lbvh_expand_bits(lbvh_quantise(c.y)) << 1 | lbvh_expand_bits(lbvh_quantise(c.z));
    indices[i] = i;
}
#endif  // ATN_SKINNING_TU

} // namespace atn
