// The TOP layer built on the device: an LBVH over the instances' world boxes (atn_tlas_rebuild, docs/TLAS.md).
//
// The stages are the bottom-level LBVH's (device/lbvh.hpp) with an instance's world box in place of a triangle's box, and
// 32-byte TLAS-leaf records in place of triangle leaves:
//
//   leaf box    local box = the root record of the instance's list AS IT IS IN THE NODE IMAGE (after a list rebuild: the new
//               root; a list that is one triangle: that triangle's vertices), world box = min / max of its eight corners
//               through the instance's L2W rows, every coordinate ((m0 x + m1 y) + m2 z) + m3 in fp32, never contracted
//   union       min / max over all leaf boxes: the box the Morton codes are normalised by
//   code        the bottom-level builder's genMortonCode expressions (k_lbvh_morton); an axis of zero extent takes coordinate 0 by an explicit select
//   sort        stable by code (ties: the leaf table's order)
//   hierarchy   findSpan / findSplit of the reference's buildTree, duplicates as k_lbvh_hierarchy handles them
//   links       apply_traverse_order: hit = left child, miss = right sibling of the nearest ancestor-or-self that is a left child
//   boxes       an inner node's box = union of the leaf boxes below it (exact: any order gives the same bits)
//   emit        2 n - 1 records at top_base: inner node i (root = 0) at top_base + 32 i, the leaf with table index k at
//               top_base + 32 (n - 1 + k) -- links are explicit, so the placement is free, and this one the host knows
//               without reading anything back
//
// min / max are written as selects (tlas_min / tlas_max) that order -0 below +0: commutative and associative on everything
// but NaN, so that every reduction order here and the sequential CPU twin the tests hold this to give the same bits.
//
// Two paths, byte-identical records:
//   k_tlas_block      n <= kTlasBlockMax: ONE launch of one workgroup, everything between the leaf boxes and the records in LDS
//                     (the case every real scene hits: the atrium has 8 instances)
//   general           k_tlas_leaf_boxes -> k_tlas_union -> k_tlas_codes -> k_radix_* x 4 -> k_lbvh_hierarchy (both lbvh.hpp's,
//                     launched by aten_amd.hip) -> k_tlas_bounds -> k_tlas_emit
#pragma once
#include "lbvh.hpp"

namespace atn {

constexpr uint32_t kTlasBlockMax = 1024;        // leaves of the block path = threads of its one workgroup

// What does not move between ticks, per KIND_TLAS leaf of the last host-given top layer (16 B)
struct TlasLeaf { int32_t objid, blas_root, twin, meshid; };
struct TlasBox { float mn[3], mx[3]; };

struct TlasArgs {
    const TlasLeaf* table;              // [n]
    uint32_t n;
    uint32_t top_base;                  // byte offset of the top layer in the node image
    float4* image;                      // the node image of the set being written: the lists' roots are read, the top layer is written
    const atn_object_param* objects;
    const float4* matrices;             // 4 rows per mat4; L2W of an instance = rows 4 mtx_id .., W2L = rows 4 (mtx_id + 1) ..
    const atn_triangle_param* tris;
    const float4* vtx_pos;
    int32_t recognise_identity;         // emit_list flags identity instances only when the host holds the matrices
    // general path only
    TlasBox* wbox;                      // [n] world boxes by table index
    TlasBox* partial;                   // [blocks of k_tlas_leaf_boxes]
    TlasBox* ubox;                      // [1]
    uint32_t n_partial;
    uint32_t* codes;                    // [n]
    uint32_t* indices;                  // [n]
    TlasBox* nbox;                      // [2n-1] node boxes (inner 0 .. n-2, sorted leaves behind)
    uint32_t* arrived;                  // [n-1], zeroed by k_lbvh_hierarchy
    LbvhTopo topo;
};

#ifdef ATN_TLAS_TU    // (the kernels: tlas.hip; aten_amd.hip reads the declarations above)
__device__ __forceinline__ float tlas_min(float a, float b) { return (a < b || (a == b && (__float_as_uint(a) >> 31))) ? a : b; }
__device__ __forceinline__ float tlas_max(float a, float b) { return (a > b || (a == b && (__float_as_uint(b) >> 31))) ? a : b; }
__device__ __forceinline__ void tlas_merge(f3& mn, f3& mx, const f3& omn, const f3& omx)
{
    mn = mk3(tlas_min(mn.x, omn.x), tlas_min(mn.y, omn.y), tlas_min(mn.z, omn.z));
    mx = mk3(tlas_max(mx.x, omx.x), tlas_max(mx.y, omx.y), tlas_max(mx.z, omx.z));
}

// ((m0 x + m1 y) + m2 z) + m3, one rounding per operation whatever the contraction flags are
__device__ __forceinline__ float tlas_row(const float4& m, float x, float y, float z)
{
    return __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(m.x, x), __fmul_rn(m.y, y)), __fmul_rn(m.z, z)), m.w);
}

// world box of the leaf with table index k
__device__ __forceinline__ void tlas_leaf_box(const TlasArgs& a, uint32_t k, f3& mn, f3& mx)
{
    const TlasLeaf lf = a.table[k];
    const float4* q = reinterpret_cast<const float4*>(reinterpret_cast<const char*>(a.image) + ((uint32_t)lf.blas_root & kLinkOffsetMask));
    f3 lmn, lmx;
    if ((lf.blas_root & kLinkTypeMask) == kLinkLeafBit) {       // the list is one triangle: its vertices as they are now
        const int32_t tri = __float_as_int(q[0].w);
        const float4 v0 = a.vtx_pos[a.tris[tri].idx[0]], v1 = a.vtx_pos[a.tris[tri].idx[1]], v2 = a.vtx_pos[a.tris[tri].idx[2]];
        lmn = mk3(tlas_min(tlas_min(v0.x, v1.x), v2.x), tlas_min(tlas_min(v0.y, v1.y), v2.y), tlas_min(tlas_min(v0.z, v1.z), v2.z));
        lmx = mk3(tlas_max(tlas_max(v0.x, v1.x), v2.x), tlas_max(tlas_max(v0.y, v1.y), v2.y), tlas_max(tlas_max(v0.z, v1.z), v2.z));
    }
    else {
        const float4 q0 = q[0], q1 = q[1];
        lmn = mk3(q0.x, q0.y, q0.z); lmx = mk3(q1.x, q1.y, q1.z);
    }
    const int32_t mtx_id = a.objects[lf.objid].mtx_id;
    if (mtx_id < 0) { mn = lmn; mx = lmx; return; }
    const float4 r0 = a.matrices[4 * mtx_id + 0], r1 = a.matrices[4 * mtx_id + 1], r2 = a.matrices[4 * mtx_id + 2];
    mn = mk3(INFINITY); mx = mk3(-INFINITY);
    for (int c = 0; c < 8; c++) {
        const float x = (c & 1) ? lmx.x : lmn.x, y = (c & 2) ? lmx.y : lmn.y, z = (c & 4) ? lmx.z : lmn.z;
        const f3 w = mk3(tlas_row(r0, x, y, z), tlas_row(r1, x, y, z), tlas_row(r2, x, y, z));
        tlas_merge(mn, mx, w, w);
    }
}

// genMortonCode's expressions over the leaf's box and the union box; a flat (or non-finite) axis takes coordinate 0
__device__ __forceinline__ uint32_t tlas_code(const f3& mn, const f3& mx, const f3& umn, const f3& umx)
{
    const f3 size = umx - umn;
    const f3 c = (mn + mx) * 0.5F;
    const float x = size.x > 0.0F ? (c.x - umn.x) / size.x : 0.0F;
    const float y = size.y > 0.0F ? (c.y - umn.y) / size.y : 0.0F;
    const float z = size.z > 0.0F ? (c.z - umn.z) / size.z : 0.0F;
    return lbvh_expand_bits(lbvh_quantise(x)) << 2 | lbvh_expand_bits(lbvh_quantise(y)) << 1 | lbvh_expand_bits(lbvh_quantise(z));
}

// typed link of node j (inner 0 .. n-2; n-1+s = the leaf at sorted position s, whose table index is idx_of(s))
template <class IdxOf>
__device__ __forceinline__ int32_t tlas_typed(int32_t j, int32_t num, uint32_t top_base, IdxOf idx_of)
{
    if (j < 0) return kLinkEnd;
    if (j < num - 1) return (int32_t)(top_base + kInnerBytes * (uint32_t)j);
    return (int32_t)(top_base + kInnerBytes * ((uint32_t)(num - 1) + idx_of(j - (num - 1)))) | kLinkToTlas;
}

// the record of the leaf with table index k; `next` = its typed hit = miss link
__device__ __forceinline__ void tlas_emit_leaf(const TlasArgs& a, uint32_t k, int32_t next)
{
    const TlasLeaf lf = a.table[k];
    const int32_t mtx_id = a.objects[lf.objid].mtx_id;
    const int32_t w2l_row = mtx_id >= 0 ? 4 * (mtx_id + 1) : -1;
    int32_t flags = 0;
    if (w2l_row >= 0 && a.recognise_identity) {
        bool ident = true;
        for (int r = 0; r < 4; r++) {
            const float4 m = a.matrices[w2l_row + r];
            const uint32_t one = 0x3f800000u;
            ident = ident && __float_as_uint(m.x) == (r == 0 ? one : 0u) && __float_as_uint(m.y) == (r == 1 ? one : 0u)
                    && __float_as_uint(m.z) == (r == 2 ? one : 0u) && __float_as_uint(m.w) == (r == 3 ? one : 0u);
        }
        if (ident) flags |= kTlasIdentity;
    }
    float4* q = reinterpret_cast<float4*>(reinterpret_cast<char*>(a.image) + a.top_base + kInnerBytes * (a.n - 1u + k));
    q[0] = make_float4(__int_as_float(lf.objid), __int_as_float(w2l_row), __int_as_float(lf.blas_root), __int_as_float(flags));
    q[1] = make_float4(__int_as_float(lf.meshid), __int_as_float(next), __int_as_float(next), __int_as_float(lf.twin));
}

// findSpan + findSplit of inner node idx over sorted codes (k_lbvh_hierarchy's body): its range [lo, hi] and its children
__device__ __forceinline__ void tlas_span_split(const uint32_t* keys, int32_t num, int32_t idx, int32_t& lo, int32_t& hi, int32_t& cl, int32_t& cr)
{
    const int32_t d = (lbvh_lcp(keys, num, idx, idx + 1) - lbvh_lcp(keys, num, idx, idx - 1)) < 0 ? -1 : 1;
    const int32_t min_lcp = lbvh_lcp(keys, num, idx, idx - d);
    int32_t lmax = 2;
    while (lbvh_lcp(keys, num, idx, idx + lmax * d) > min_lcp) lmax *= 2;
    int32_t l = 0, s = lmax;
    do {
        s /= 2;
        if (lbvh_lcp(keys, num, idx, idx + (l + s) * d) > min_lcp) l += s;
    } while (s > 1);
    lo = min(idx, idx + l * d); hi = max(idx, idx + l * d);
    int32_t left = lo, right = hi;
    const int32_t identical = lbvh_lcp(keys, num, left, right);
    do {
        const int32_t mid = (right + left) / 2;
        if (lbvh_lcp(keys, num, left, mid) > identical) left = mid;
        else right = mid;
    } while (right > left + 1);
    const int32_t split = left;
    cl = split == lo ? split + num - 1 : split;
    cr = split + 1 == hi ? split + 1 + num - 1 : split + 1;
}

// ---------------------------------------------------------------------------------------------------------------------
// The block path: 2 <= n <= kTlasBlockMax, one workgroup of `blockDim.x` = a power of two >= n threads, thread t = the leaf
// with table index t before the sort and the leaf at sorted position t after it.  76 KB of LDS (gfx950: 160 KB per workgroup).
__global__ __launch_bounds__(kTlasBlockMax) void k_tlas_block(TlasArgs a)
{
    __shared__ unsigned long long keys[kTlasBlockMax];          // code << 32 | table index: unique, so any sort is the stable sort by code
    __shared__ uint32_t codes[kTlasBlockMax];
    __shared__ int32_t parent[2 * kTlasBlockMax - 1], left[kTlasBlockMax - 1], right[kTlasBlockMax - 1];
    __shared__ float nbox[6][2 * kTlasBlockMax - 1];
    __shared__ uint32_t arrived[kTlasBlockMax - 1];
    __shared__ float red[6][kTlasBlockMax / 64];
    const int32_t tid = threadIdx.x, num = (int32_t)a.n;
    const bool valid = tid < num;
    f3 mn = mk3(INFINITY), mx = mk3(-INFINITY);
    if (valid) tlas_leaf_box(a, (uint32_t)tid, mn, mx);
    {   // the union box: a wave's by shuffles, the workgroup's through LDS; every thread folds the waves' boxes itself
        f3 wmn = mn, wmx = mx;
        for (int d = 32; d > 0; d >>= 1)
            tlas_merge(wmn, wmx, mk3(__shfl_xor(wmn.x, d), __shfl_xor(wmn.y, d), __shfl_xor(wmn.z, d)), mk3(__shfl_xor(wmx.x, d), __shfl_xor(wmx.y, d), __shfl_xor(wmx.z, d)));
        if ((tid & 63) == 0) {
            const int w = tid >> 6;
            red[0][w] = wmn.x; red[1][w] = wmn.y; red[2][w] = wmn.z; red[3][w] = wmx.x; red[4][w] = wmx.y; red[5][w] = wmx.z;
        }
    }
    __syncthreads();
    f3 umn = mk3(INFINITY), umx = mk3(-INFINITY);
    for (uint32_t w = 0; w < blockDim.x / 64u; w++) tlas_merge(umn, umx, mk3(red[0][w], red[1][w], red[2][w]), mk3(red[3][w], red[4][w], red[5][w]));
    keys[tid] = valid ? ((unsigned long long)tlas_code(mn, mx, umn, umx) << 32 | (unsigned long long)(uint32_t)tid) : ~0ull;
    __syncthreads();
    // bitonic sort of blockDim.x keys (the padding sorts to the end)
    for (uint32_t k = 2; k <= blockDim.x; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            const uint32_t other = (uint32_t)tid ^ j;
            if (other > (uint32_t)tid) {
                const unsigned long long x = keys[tid], y = keys[other];
                const bool up = ((uint32_t)tid & k) == 0u;
                if ((x > y) == up) { keys[tid] = y; keys[other] = x; }
            }
            __syncthreads();
        }
    const uint32_t my_idx = (uint32_t)keys[tid];                // table index of the leaf at sorted position tid
    codes[tid] = (uint32_t)(keys[tid] >> 32);
    if (tid == 0) parent[0] = -1;
    __syncthreads();
    if (tid < num - 1) {
        int32_t lo, hi, cl, cr;
        tlas_span_split(codes, num, tid, lo, hi, cl, cr);
        left[tid] = cl; right[tid] = cr;
        parent[cl] = tid; parent[cr] = tid;
        arrived[tid] = 0;
    }
    __syncthreads();
    // boxes: the reference's climb, the second child to arrive at a node merges (workgroup-scope hand-overs)
    if (valid) {
        tlas_leaf_box(a, my_idx, mn, mx);           // (recomputed from the same inputs: the same bits as before the sort)
        int32_t cur = tid + num - 1;
        for (;;) {
            nbox[0][cur] = mn.x; nbox[1][cur] = mn.y; nbox[2][cur] = mn.z; nbox[3][cur] = mx.x; nbox[4][cur] = mx.y; nbox[5][cur] = mx.z;
            const int32_t p = parent[cur];
            if (p < 0) break;
            if (__hip_atomic_fetch_add(&arrived[p], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP) == 0u) break;
            const int32_t o = left[p] == cur ? right[p] : left[p];
            tlas_merge(mn, mx, mk3(nbox[0][o], nbox[1][o], nbox[2][o]), mk3(nbox[3][o], nbox[4][o], nbox[5][o]));
            cur = p;
        }
    }
    __syncthreads();
    // links and records
    auto idx_of = [&](int32_t s) { return (uint32_t)keys[s]; };
    for (int32_t node = tid; node < 2 * num - 1; node += (int32_t)blockDim.x) {
        int32_t miss = -1;
        for (int32_t cur = node;;) {
            const int32_t p = parent[cur];
            if (p < 0) break;
            if (left[p] == cur) { miss = right[p]; break; }
            cur = p;
        }
        const int32_t tm = tlas_typed(miss, num, a.top_base, idx_of);
        if (node < num - 1) {
            float4* q = reinterpret_cast<float4*>(reinterpret_cast<char*>(a.image) + a.top_base + kInnerBytes * (uint32_t)node);
            q[0] = make_float4(nbox[0][node], nbox[1][node], nbox[2][node], __int_as_float(tlas_typed(left[node], num, a.top_base, idx_of)));
            q[1] = make_float4(nbox[3][node], nbox[4][node], nbox[5][node], __int_as_float(tm));
        }
        else tlas_emit_leaf(a, idx_of(node - (num - 1)), tm);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// The general path.
__global__ __launch_bounds__(256) void k_tlas_leaf_boxes(TlasArgs a)
{
    __shared__ float red[6][4];
    const uint32_t tid = threadIdx.x, i = blockIdx.x * 256u + tid;
    f3 mn = mk3(INFINITY), mx = mk3(-INFINITY);
    if (i < a.n) {
        tlas_leaf_box(a, i, mn, mx);
        TlasBox& b = a.wbox[i];
        b.mn[0] = mn.x; b.mn[1] = mn.y; b.mn[2] = mn.z; b.mx[0] = mx.x; b.mx[1] = mx.y; b.mx[2] = mx.z;
    }
    for (int d = 32; d > 0; d >>= 1)
        tlas_merge(mn, mx, mk3(__shfl_xor(mn.x, d), __shfl_xor(mn.y, d), __shfl_xor(mn.z, d)), mk3(__shfl_xor(mx.x, d), __shfl_xor(mx.y, d), __shfl_xor(mx.z, d)));
    if ((tid & 63u) == 0u) {
        const uint32_t w = tid >> 6;
        red[0][w] = mn.x; red[1][w] = mn.y; red[2][w] = mn.z; red[3][w] = mx.x; red[4][w] = mx.y; red[5][w] = mx.z;
    }
    __syncthreads();
    if (tid == 0) {
        for (uint32_t w = 1; w < 4; w++) tlas_merge(mn, mx, mk3(red[0][w], red[1][w], red[2][w]), mk3(red[3][w], red[4][w], red[5][w]));
        TlasBox& b = a.partial[blockIdx.x];
        b.mn[0] = mn.x; b.mn[1] = mn.y; b.mn[2] = mn.z; b.mx[0] = mx.x; b.mx[1] = mx.y; b.mx[2] = mx.z;
    }
}

// one workgroup: the blocks' boxes -> the union box
__global__ __launch_bounds__(256) void k_tlas_union(TlasArgs a)
{
    __shared__ float red[6][4];
    const uint32_t tid = threadIdx.x;
    f3 mn = mk3(INFINITY), mx = mk3(-INFINITY);
    for (uint32_t i = tid; i < a.n_partial; i += 256u) {
        const TlasBox b = a.partial[i];
        tlas_merge(mn, mx, mk3(b.mn[0], b.mn[1], b.mn[2]), mk3(b.mx[0], b.mx[1], b.mx[2]));
    }
    for (int d = 32; d > 0; d >>= 1)
        tlas_merge(mn, mx, mk3(__shfl_xor(mn.x, d), __shfl_xor(mn.y, d), __shfl_xor(mn.z, d)), mk3(__shfl_xor(mx.x, d), __shfl_xor(mx.y, d), __shfl_xor(mx.z, d)));
    if ((tid & 63u) == 0u) {
        const uint32_t w = tid >> 6;
        red[0][w] = mn.x; red[1][w] = mn.y; red[2][w] = mn.z; red[3][w] = mx.x; red[4][w] = mx.y; red[5][w] = mx.z;
    }
    __syncthreads();
    if (tid == 0) {
        for (uint32_t w = 1; w < 4; w++) tlas_merge(mn, mx, mk3(red[0][w], red[1][w], red[2][w]), mk3(red[3][w], red[4][w], red[5][w]));
        TlasBox& b = a.ubox[0];
        b.mn[0] = mn.x; b.mn[1] = mn.y; b.mn[2] = mn.z; b.mx[0] = mx.x; b.mx[1] = mx.y; b.mx[2] = mx.z;
    }
}

__global__ __launch_bounds__(256) void k_tlas_codes(TlasArgs a)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.n) return;
    const TlasBox b = a.wbox[i], u = a.ubox[0];
    a.codes[i] = tlas_code(mk3(b.mn[0], b.mn[1], b.mn[2]), mk3(b.mx[0], b.mx[1], b.mx[2]), mk3(u.mn[0], u.mn[1], u.mn[2]), mk3(u.mx[0], u.mx[1], u.mx[2]));
    a.indices[i] = i;
}

// The reference's climb over the whole device: one thread per sorted leaf, the second child to arrive at a node merges.  The
// hand-overs are agent-scope (a write-back per hand-over: device/lbvh.hpp measured what that costs at 10^6 leaves and does
// without); a top layer beyond kTlasBlockMax instances is rare and a few thousand leaves at most in practice.
__global__ __launch_bounds__(256) void k_tlas_bounds(TlasArgs a)
{
    const int32_t i = blockIdx.x * 256 + threadIdx.x, num = (int32_t)a.n;
    if (i >= num) return;
    const TlasBox b = a.wbox[a.indices[i]];
    f3 mn = mk3(b.mn[0], b.mn[1], b.mn[2]), mx = mk3(b.mx[0], b.mx[1], b.mx[2]);
    int32_t cur = i + num - 1;
    for (;;) {
        TlasBox& g = a.nbox[cur];
        g.mn[0] = mn.x; g.mn[1] = mn.y; g.mn[2] = mn.z; g.mx[0] = mx.x; g.mx[1] = mx.y; g.mx[2] = mx.z;
        const int32_t p = a.topo.parent[cur];
        if (p < 0) return;
        if (__hip_atomic_fetch_add(&a.arrived[p], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == 0u) return;
        const TlasBox o = a.nbox[a.topo.left[p] == cur ? a.topo.right[p] : a.topo.left[p]];
        tlas_merge(mn, mx, mk3(o.mn[0], o.mn[1], o.mn[2]), mk3(o.mx[0], o.mx[1], o.mx[2]));
        cur = p;
    }
}

__global__ __launch_bounds__(256) void k_tlas_emit(TlasArgs a)
{
    const int32_t node = blockIdx.x * 256 + threadIdx.x, num = (int32_t)a.n;
    if (node >= 2 * num - 1) return;
    auto idx_of = [&](int32_t s) { return a.indices[s]; };
    int32_t miss = -1;
    for (int32_t cur = node;;) {
        const int32_t p = a.topo.parent[cur];
        if (p < 0) break;
        if (a.topo.left[p] == cur) { miss = a.topo.right[p]; break; }
        cur = p;
    }
    const int32_t tm = tlas_typed(miss, num, a.top_base, idx_of);
    if (node < num - 1) {
        const TlasBox b = a.nbox[node];
        float4* q = reinterpret_cast<float4*>(reinterpret_cast<char*>(a.image) + a.top_base + kInnerBytes * (uint32_t)node);
        q[0] = make_float4(b.mn[0], b.mn[1], b.mn[2], __int_as_float(tlas_typed(a.topo.left[node], num, a.top_base, idx_of)));
        q[1] = make_float4(b.mx[0], b.mx[1], b.mx[2], __int_as_float(tm));
    }
    else tlas_emit_leaf(a, idx_of(node - (num - 1)), tm);
}

#endif  // ATN_TLAS_TU

} // namespace atn
