/*
 * TEST INFRASTRUCTURE ONLY: the CPU twin of the device-built top layer (atn_tlas_rebuild, aten_amd/csrc/device/tlas.hpp,
 * docs/TLAS.md).  It restates the pinned arithmetic -- world boxes, union box, Morton codes -- sequentially, and takes the sort,
 * the hierarchy and the threading from oracle/orc_lbvh.h unchanged (computeMortonCode, sort_by_key, build_tree,
 * apply_traverse_order).  The product never includes this file.
 *
 * Built two ways (tests/tlas_oracle.py, tests/test_tlas_oracle_cpu.py):
 *   g++ -shared                                   orc_tlas_build for ctypes
 *   g++ -DTLAS_ORACLE_MAIN -fsanitize=address,undefined   a stand-alone program: random and degenerate instance sets through
 *                                                 orc_tlas_build and the structural checks, "ok" and exit status 0
 */
#include "../../oracle/orc_lbvh.h"
#include <cstdio>
#include <cstring>
#include <limits>

namespace {

inline uint32_t fbits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
// min / max as selects that order -0 below +0 (device/tlas.hpp: tlas_min / tlas_max)
inline float tmin(float a, float b) { return (a < b || (a == b && (fbits(a) >> 31))) ? a : b; }
inline float tmax(float a, float b) { return (a > b || (a == b && (fbits(b) >> 31))) ? a : b; }
// ((m0 x + m1 y) + m2 z) + m3, left to right (built with -ffp-contract=off)
inline float row(const float m[4], float x, float y, float z)
{
    float r = m[0] * x;
    const float s = m[1] * y;
    r = r + s;
    const float t = m[2] * z;
    r = r + t;
    r = r + m[3];
    return r;
}

}  // namespace

extern "C" {

/* payload: per leaf, in the leaf table's order, the four payload floats of the host top layer's leaf (f0 = objid, f1, f2 = exid
 * bits, f3 = meshid).  local: per leaf {min xyz, max xyz} of its list's root.  Outputs: world [n][6], sorted codes and indices
 * [n], nodes [2n - 1] in the reference's node order (inner 0 .. n-2, leaves n-1 .. 2n-2 by sorted position).
 * Returns 0, or -1 for an id out of range. */
int orc_tlas_build(const float* payload, uint32_t n, const atn_object_param* objects, uint32_t n_objects,
                   const atn_mat4* matrices, uint32_t n_matrices, const float* local,
                   float* out_world, uint32_t* out_codes, uint32_t* out_indices, atn_bvh_node* out_nodes)
{
    if (n == 0) return -1;
    const float inf = std::numeric_limits<float>::infinity();
    std::vector<float> world(6 * (size_t)n);
    float umn[3] = { inf, inf, inf }, umx[3] = { -inf, -inf, -inf };
    for (uint32_t k = 0; k < n; k++) {
        const int32_t objid = (int32_t)payload[4 * k];
        if (objid < 0 || (uint32_t)objid >= n_objects) return -1;
        const int32_t mtx_id = objects[objid].mtx_id;
        const float* l = local + 6 * (size_t)k;
        float* w = &world[6 * (size_t)k];
        if (mtx_id < 0) std::memcpy(w, l, 6 * sizeof(float));
        else {
            if ((uint32_t)mtx_id + 1 >= n_matrices) return -1;
            const atn_mat4& m = matrices[mtx_id];       // L2W (W2L follows it)
            for (int a = 0; a < 3; a++) { w[a] = inf; w[3 + a] = -inf; }
            for (int c = 0; c < 8; c++) {
                const float x = (c & 1) ? l[3] : l[0], y = (c & 2) ? l[4] : l[1], z = (c & 4) ? l[5] : l[2];
                for (int a = 0; a < 3; a++) {
                    const float v = row(m.m[a], x, y, z);
                    w[a] = tmin(w[a], v); w[3 + a] = tmax(w[3 + a], v);
                }
            }
        }
        for (int a = 0; a < 3; a++) { umn[a] = tmin(umn[a], w[a]); umx[a] = tmax(umx[a], w[3 + a]); }
    }
    // gen_morton's expressions with the instance's world box in place of the triangle's; a flat axis takes coordinate 0
    std::vector<uint32_t> codes(n), indices(n);
    const float size[3] = { umx[0] - umn[0], umx[1] - umn[1], umx[2] - umn[2] };
    for (uint32_t k = 0; k < n; k++) {
        const float* w = &world[6 * (size_t)k];
        float c[3];
        for (int a = 0; a < 3; a++) {
            c[a] = (w[a] + w[3 + a]) * 0.5f;
            c[a] = size[a] > 0.0f ? (c[a] - umn[a]) / size[a] : 0.0f;
        }
        codes[k] = orc::lbvh::computeMortonCode(c[0], c[1], c[2]);
        indices[k] = k;
    }
    orc::lbvh::sort_by_key(codes, indices);
    auto leaf = [&](atn_bvh_node& g, uint32_t k) {
        const float* w = &world[6 * (size_t)k];
        for (int a = 0; a < 3; a++) { g.boxmin[a] = w[a]; g.boxmax[a] = w[3 + a]; }
        g.f0 = payload[4 * k]; g.f1 = payload[4 * k + 1]; g.f2 = payload[4 * k + 2]; g.f3 = payload[4 * k + 3];
    };
    if (n == 1) {       // (the reference's buildTree leaves one leaf alone: the layer is that leaf)
        std::memset(&out_nodes[0], 0, sizeof(atn_bvh_node));
        out_nodes[0].hit = -1; out_nodes[0].miss = -1;
        leaf(out_nodes[0], 0);
    }
    else {
        std::vector<orc::lbvh::Node> nodes;
        orc::lbvh::build_tree(codes.data(), n, nodes);
        for (int32_t i = 0; i < (int32_t)(2 * n - 1); i++) orc::lbvh::apply_traverse_order(i, (int32_t)n, 0, nodes, indices.data(), out_nodes);
        for (uint32_t s = 0; s < n; s++) leaf(out_nodes[n - 1 + s], indices[s]);
        // inner boxes = unions of the children's, post order (explicit stack: LBVH trees can be deep)
        std::vector<int32_t> stack{ 0 };
        std::vector<uint8_t> expanded(nodes.size(), 0);
        while (!stack.empty()) {
            const int32_t i = stack.back();
            if (nodes[i].isLeaf) { stack.pop_back(); continue; }
            if (!expanded[i]) { expanded[i] = 1; stack.push_back(nodes[i].left); stack.push_back(nodes[i].right); continue; }
            stack.pop_back();
            const atn_bvh_node& a = out_nodes[nodes[i].left];
            const atn_bvh_node& b = out_nodes[nodes[i].right];
            for (int k = 0; k < 3; k++) {
                out_nodes[i].boxmin[k] = tmin(a.boxmin[k], b.boxmin[k]);
                out_nodes[i].boxmax[k] = tmax(a.boxmax[k], b.boxmax[k]);
            }
        }
    }
    if (out_world) std::memcpy(out_world, world.data(), world.size() * sizeof(float));
    if (out_codes) std::memcpy(out_codes, codes.data(), n * sizeof(uint32_t));
    if (out_indices) std::memcpy(out_indices, indices.data(), n * sizeof(uint32_t));
    return 0;
}

/* The structure a threaded top layer must have: following hit links from node 0 reaches every leaf exactly once, every link
 * points forward in that order, and every inner box equals the union of the boxes of the leaves below it (= the leaves between
 * the node and its miss link).  Returns 0, or the number of the first rule that fails. */
int orc_tlas_check(const atn_bvh_node* nodes, uint32_t n_leaves)
{
    const uint32_t count = 2 * n_leaves - 1;
    std::vector<int32_t> pos(count, -1);
    std::vector<uint32_t> order;
    for (int32_t id = 0; id >= 0;) {
        if ((uint32_t)id >= count || pos[id] >= 0) return 1;
        pos[id] = (int32_t)order.size();
        order.push_back((uint32_t)id);
        id = (int32_t)nodes[id].hit;
    }
    if (order.size() != count) return 2;
    uint32_t leaves = 0;
    for (uint32_t j = 0; j < count; j++) {
        const atn_bvh_node& nd = nodes[order[j]];
        const bool leaf = nd.f0 >= 0 || nd.f1 >= 0;
        leaves += leaf ? 1u : 0u;
        for (const float link : { nd.hit, nd.miss }) {
            const int32_t l = (int32_t)link;
            if (l >= 0 && ((uint32_t)l >= count || pos[l] <= (int32_t)j)) return 3;
        }
        if (leaf) continue;
        const uint32_t end = (int32_t)nd.miss < 0 ? count : (uint32_t)pos[(int32_t)nd.miss];
        const float inf = std::numeric_limits<float>::infinity();
        float mn[3] = { inf, inf, inf }, mx[3] = { -inf, -inf, -inf };
        for (uint32_t k = j + 1; k < end; k++) {
            const atn_bvh_node& c = nodes[order[k]];
            if (!(c.f0 >= 0 || c.f1 >= 0)) continue;
            for (int a = 0; a < 3; a++) { mn[a] = tmin(mn[a], c.boxmin[a]); mx[a] = tmax(mx[a], c.boxmax[a]); }
        }
        if (std::memcmp(mn, nd.boxmin, sizeof(mn)) != 0 || std::memcmp(mx, nd.boxmax, sizeof(mx)) != 0) return 4;
    }
    return leaves == n_leaves ? 0 : 5;
}

}  // extern "C"

#ifdef TLAS_ORACLE_MAIN
namespace {

uint32_t rng_state = 12345u;
float rnd() { rng_state = rng_state * 1664525u + 1013904223u; return (float)(rng_state >> 8) * (1.0f / 16777216.0f); }

// n instances of one unit quad: random rigid placements, one instance without a matrix, one exact identity
int run(uint32_t n, int kind)
{
    std::vector<atn_object_param> objects(n + 1);
    std::vector<atn_mat4> matrices(2 * (size_t)n + 2);
    std::vector<float> payload(4 * (size_t)n), local(6 * (size_t)n);
    std::memset(objects.data(), 0, objects.size() * sizeof(atn_object_param));
    std::memset(matrices.data(), 0, matrices.size() * sizeof(atn_mat4));
    for (uint32_t k = 0; k < n; k++) {
        atn_object_param& o = objects[k + 1];
        o.type = ATN_OBJ_INSTANCE; o.object_id = 0; o.mtx_id = (k == 1 && n > 2) ? -1 : (int32_t)(2 * k);
        atn_mat4& m = matrices[2 * (size_t)k];
        const float ang = kind == 0 ? rnd() * 6.28f : 0.0f, c = std::cos(ang), s = std::sin(ang);
        const float t[3] = { kind == 1 ? 1.0f : rnd() * 20.0f - 10.0f, kind == 1 ? 2.0f : rnd() * 20.0f - 10.0f, kind == 0 ? rnd() * 20.0f - 10.0f : 3.0f };
        const float rot[4][4] = { { c, 0, s, t[0] }, { 0, 1, 0, t[1] }, { -s, 0, c, t[2] }, { 0, 0, 0, 1 } };
        std::memcpy(m.m, rot, sizeof(rot));
        if (k == 2 && kind == 0) { const float I[4][4] = { { 1, 0, 0, 0 }, { 0, 1, 0, 0 }, { 0, 0, 1, 0 }, { 0, 0, 0, 1 } }; std::memcpy(m.m, I, sizeof(I)); }
        const uint32_t exid = 1;
        payload[4 * k] = (float)(k + 1); payload[4 * k + 1] = -1.0f; std::memcpy(&payload[4 * k + 2], &exid, 4); payload[4 * k + 3] = 0.0f;
        const float box[6] = { -0.5f, -0.5f, 0.0f, 0.5f, 0.5f, 0.0f };
        std::memcpy(&local[6 * (size_t)k], box, sizeof(box));
    }
    std::vector<float> world(6 * (size_t)n);
    std::vector<uint32_t> codes(n), indices(n);
    std::vector<atn_bvh_node> nodes(2 * (size_t)n - 1);
    if (orc_tlas_build(payload.data(), n, objects.data(), (uint32_t)objects.size(), matrices.data(), (uint32_t)matrices.size(), local.data(),
                       world.data(), codes.data(), indices.data(), nodes.data()) != 0) return 100;
    for (uint32_t k = 1; k < n; k++) if (codes[k - 1] > codes[k] || (codes[k - 1] == codes[k] && indices[k - 1] > indices[k])) return 101;
    return orc_tlas_check(nodes.data(), n);
}

}  // namespace

int main()
{
    const uint32_t sizes[] = { 1, 2, 3, 7, 64, 65, 1024, 1025, 4097 };
    for (const uint32_t n : sizes) {
        const int rc = run(n, 0);
        if (rc) { std::printf("n = %u: rule %d\n", n, rc); return 1; }
    }
    for (int kind = 1; kind <= 2; kind++) {     // every box identical; every centre in one plane
        const int rc = run(300, kind);
        if (rc) { std::printf("degenerate set %d: rule %d\n", kind, rc); return 1; }
    }
    // refusals
    {
        const float payload[4] = { 5.0f, -1.0f, 0.0f, 0.0f }, local[6] = { 0, 0, 0, 1, 1, 1 };
        atn_object_param o{};
        atn_bvh_node out[1];
        if (orc_tlas_build(payload, 1, &o, 1, nullptr, 0, local, nullptr, nullptr, nullptr, out) != -1) { std::printf("an object id out of range was accepted\n"); return 1; }
    }
    std::printf("ok\n");
    return 0;
}
#endif
