// Host-side unit test of the sphere leaves of the upload (aten_amd/csrc/host/scene_upload.hpp: pure host C++, compiled with hipcc for
// its headers only -- no HIP call is made, no GPU is needed; docs/SPHERES.md).  A hand-written scene: one triangle in a bottom-level
// list, and a top layer  root (inner) -> instance leaf -> sphere leaf.
//   * sphere_mode 0: the image is byte-equal to an upload through the argument list that has no such mode
//   * sphere_mode 1: the image differs from it only in the sphere leaf's record and in the links that name it; the record holds
//     {center, radius}{objid, sphere.mtrl_id, meshid, next link}
//   * each refusal fires: an instance of a sphere, hit != miss, such a leaf in a bottom-level list, an object id out of range
// Prints "ok" or the first thing that is wrong (exit code 1).
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../aten_amd/csrc/host/scene_upload.hpp"

using namespace atn;

static int fail(const std::string& what) { std::printf("FAILED: %s\n", what.c_str()); return 1; }
static int32_t f2i_(float f) { int32_t i; std::memcpy(&i, &f, 4); return i; }

static atn_bvh_node node(float hit, float miss, float f0, float f1, float f2, float f3, float lo, float hi)
{
    atn_bvh_node n{};
    for (int a = 0; a < 3; a++) { n.boxmin[a] = lo; n.boxmax[a] = hi; }
    n.hit = hit; n.miss = miss; n.f0 = f0; n.f1 = f1; n.f2 = f2; n.f3 = f3;
    return n;
}

struct Scene {
    std::vector<atn_vec4> pos, nml;
    std::vector<atn_triangle_param> tris;
    std::vector<atn_object_param> objs;
    std::vector<atn_mat4> mtx;
    std::vector<atn_material_param> mats;
    std::vector<atn_light_param> lights;
    std::vector<atn_bvh_node> blas, tlas;
    std::vector<atn_bvh_list> lists;
    atn_scene_desc d{};
    void finish()
    {
        lists = { { tlas.data(), (uint32_t)tlas.size(), 0 }, { blas.data(), (uint32_t)blas.size(), 0 } };
        d = atn_scene_desc{};
        d.objects = objs.data(); d.n_objects = (uint32_t)objs.size();
        d.matrices = mtx.data(); d.n_matrices = (uint32_t)mtx.size();
        d.materials = mats.data(); d.n_materials = (uint32_t)mats.size();
        d.lights = lights.data(); d.n_lights = (uint32_t)lights.size();
        d.triangles = tris.data(); d.n_triangles = (uint32_t)tris.size();
        d.vtx_pos = pos.data(); d.vtx_nml = nml.data(); d.n_vertices = (uint32_t)pos.size();
        d.bvh_lists = lists.data(); d.n_bvh_lists = (uint32_t)lists.size();
        for (int a = 0; a < 3; a++) { d.scene_bbox_min[a] = -2.f; d.scene_bbox_max[a] = 2.f; }
        d.config.bg.envmap_tex_idx = -1;
    }
};

static void make_scene(Scene& s)
{
    s.pos = { { 0, 0, 0, 0 }, { 1, 0, 0, 0 }, { 0, 1, 0, 0 } };
    s.nml = { { 0, 0, 1, 0 }, { 0, 0, 1, 0 }, { 0, 0, 1, 0 } };
    atn_triangle_param t{}; t.idx[0] = 0; t.idx[1] = 1; t.idx[2] = 2; t.area = 0.5f; t.mtrlid = 0; t.mesh_id = 0;
    s.tris = { t };
    atn_object_param poly{}; poly.type = ATN_OBJ_POLYGONS; poly.object_id = -1; poly.mtx_id = -1; poly.triangle_id = 0; poly.triangle_num = 1; poly.light_id = -1;
    atn_object_param inst{}; inst.type = ATN_OBJ_INSTANCE; inst.object_id = 0; inst.mtx_id = 0; inst.triangle_id = -1; inst.light_id = -1;
    atn_object_param sph{}; sph.type = ATN_OBJ_SPHERE; sph.object_id = -1; sph.mtx_id = -1; sph.triangle_id = -1; sph.light_id = -1;
    sph.sphere.center[0] = 0.25f; sph.sphere.center[1] = -0.5f; sph.sphere.center[2] = 1.5f; sph.sphere.radius = 0.375f; sph.sphere.mtrl_id = 1;
    atn_object_param sinst = inst; sinst.object_id = 2;         // an INSTANCE of the sphere: never a sphere leaf
    s.objs = { poly, inst, sph, sinst };
    atn_mat4 I{};
    for (int a = 0; a < 4; a++) I.m[a][a] = 1.f;
    s.mtx = { I, I };
    s.mats.resize(2);
    for (auto& m : s.mats) { std::memset(&m, 0, sizeof(m)); m.type = ATN_MTRL_DIFFUSE; m.albedoMap = m.normalMap = m.roughnessMap = -1; m.baseColor.w = 1.f; }
    // bottom-level list 1: one triangle leaf (f0 = object, f1 = triangle)
    s.blas = { node(-1, -1, 0, 0, -1, 0, 0.f, 1.f) };
    // top layer: 0 inner -> 1 instance leaf (object 1, list 1) -> 2 sphere leaf (object 2, mesh id 7)
    float exid; const uint32_t bits = 1u; std::memcpy(&exid, &bits, 4);
    s.tlas = { node(1, -1, -1, -1, -1, -1, -2.f, 2.f), node(2, 2, 1, -1, exid, 3, 0.f, 1.f), node(-1, -1, 2, -1, -1, 7, -1.f, 2.f) };
    s.finish();
}

int main()
{
    std::string err;
    Scene s; make_scene(s);
    HostSceneImage plain, m0, m1;
    // an upload that never heard of the switch: the argument list without it
    if (!build_host_image(plain, &s.d, err, 0, 8, kLayoutTopLevels, true)) return fail("plain upload: " + err);
    if (!build_host_image(m0, &s.d, err, 0, 8, kLayoutTopLevels, true, kTwinBudgetBytes, 0)) return fail("mode 0 upload: " + err);
    if (!build_host_image(m1, &s.d, err, 0, 8, kLayoutTopLevels, true, kTwinBudgetBytes, 1)) return fail("mode 1 upload: " + err);
    if (plain.nodes.size() != m0.nodes.size() || std::memcmp(plain.nodes.data(), m0.nodes.data(), plain.nodes.size() * 16) != 0) return fail("mode 0 image differs from the plain upload's");
    auto same_params = [](const DevScene& a, const DevScene& b) {      // (the walk's scalars; the struct has padding, so no memcmp)
        return a.root_link == b.root_link && a.node_bytes == b.node_bytes && a.ident_row == b.ident_row && a.root_direct == b.root_direct
            && a.root_blas == b.root_blas && a.root_objid == b.root_objid && a.material_set == b.material_set && a.any_alpha == b.any_alpha;
    };
    if (!same_params(plain.params, m0.params)) return fail("mode 0 parameters differ from the plain upload's");
    if (m0.n_sphere_leaf != 0 || plain.n_sphere_leaf != 0) return fail("mode 0 counts sphere leaves");
    if (m1.n_sphere_leaf != 1) return fail("mode 1 counts " + std::to_string(m1.n_sphere_leaf) + " sphere leaves, not 1");
    if (m1.nodes.size() != m0.nodes.size()) return fail("mode 1 image has another size");
    if (!same_params(m0.params, m1.params)) return fail("mode 1 changes the scene parameters");
    // image: [list 1: one 48-byte triangle leaf][top layer in walk order: inner, TLAS leaf, sphere leaf -- 32 bytes each]
    const uint32_t top = 48, leaf_off = top + 64;
    const float4* q = m1.nodes.data() + leaf_off / 16;
    if (q[0].x != 0.25f || q[0].y != -0.5f || q[0].z != 1.5f || q[0].w != 0.375f) return fail("sphere record: {center, radius}");
    if (f2i_(q[1].x) != 2 || f2i_(q[1].y) != 1 || f2i_(q[1].z) != 7 || f2i_(q[1].w) != kLinkEnd) return fail("sphere record: {objid, mtrl_id, meshid, link}");
    // the dead leaf of mode 0 at the same place: an inner record whose both links are the miss link
    const float4* d0 = m0.nodes.data() + leaf_off / 16;
    if (f2i_(d0[0].w) != kLinkEnd || f2i_(d0[1].w) != kLinkEnd || d0[0].x != 0.f) return fail("mode 0 dead leaf");
    // the links that name the leaf: the instance leaf's two top links
    const float4* tl1 = m1.nodes.data() + (top + 32) / 16;
    const float4* tl0 = m0.nodes.data() + (top + 32) / 16;
    if (f2i_(tl1[1].y) != (int32_t)(leaf_off | (uint32_t)kLinkToSphere) || f2i_(tl1[1].z) != f2i_(tl1[1].y)) return fail("the instance leaf's links do not name a sphere leaf");
    if (f2i_(tl0[1].y) != (int32_t)leaf_off) return fail("mode 0: the instance leaf's links");
    if ((f2i_(tl1[1].y) & kLinkTypeMask) != kLinkTypeMask || f2i_(tl1[1].y) == kLinkEnd || f2i_(tl1[1].y) >= 0) return fail("sphere link type bits");
    // everything else is byte-equal
    for (size_t i = 0; i < m0.nodes.size(); i++) {
        const size_t off = i * 16;
        const bool may_differ = (off >= leaf_off && off < leaf_off + 32) || off == top + 32 + 16;
        if (!may_differ && std::memcmp(&m0.nodes[i], &m1.nodes[i], 16) != 0) return fail("mode 1 image differs at byte " + std::to_string(off));
    }
    // a one-leaf top layer whose leaf is a sphere starts at root_link: no direct start
    {
        Scene o; make_scene(o);
        o.tlas = { node(-1, -1, 2, -1, -1, 7, -1.f, 2.f) };
        o.finish();
        HostSceneImage im;
        if (!build_host_image(im, &o.d, err, 0, 8, kLayoutTopLevels, true, kTwinBudgetBytes, 1)) return fail("one-leaf upload: " + err);
        if (im.params.root_direct != 0 || im.params.root_link != (int32_t)(48u | (uint32_t)kLinkToSphere) || im.n_sphere_leaf != 1) return fail("one-leaf top layer");
    }
    // refusals
    auto refused = [&](Scene& b, const char* what, const char* word) -> bool {
        b.finish();
        HostSceneImage im; std::string e;
        if (build_host_image(im, &b.d, e, 0, 8, kLayoutTopLevels, true, kTwinBudgetBytes, 1)) { std::printf("FAILED: %s was not refused\n", what); return false; }
        if (e.find(word) == std::string::npos || e.find("leaf") == std::string::npos) { std::printf("FAILED: %s: message '%s'\n", what, e.c_str()); return false; }
        HostSceneImage ok; std::string e0;
        if (!build_host_image(ok, &b.d, e0, 0, 8, kLayoutTopLevels, true, kTwinBudgetBytes, 0)) { std::printf("FAILED: %s is refused in mode 0 too: %s\n", what, e0.c_str()); return false; }
        return true;
    };
    { Scene b; make_scene(b); b.tlas[2].f0 = 3; if (!refused(b, "an instance of a sphere", "ATN_OBJ_SPHERE")) return 1; }
    { Scene b; make_scene(b); b.tlas[2].f0 = 0; if (!refused(b, "a polygon object's dead leaf", "ATN_OBJ_SPHERE")) return 1; }
    { Scene b; make_scene(b); b.tlas.push_back(node(-1, -1, 1, -1, b.tlas[1].f2, 3, 0.f, 1.f)); b.tlas[2].hit = 3; b.tlas[1].hit = 2; b.tlas[1].miss = 2;
      if (!refused(b, "hit != miss", "hit != miss")) return 1; }
    { Scene b; make_scene(b); b.blas = { node(1, -1, -1, -1, -1, -1, 0.f, 1.f), node(2, 2, 2, -1, -1, 0, 0.f, 1.f), node(-1, -1, 0, 0, -1, 0, 0.f, 1.f) };
      if (!refused(b, "a sphere leaf in a bottom-level list", "top layer")) return 1; }
    { Scene b; make_scene(b); b.tlas[2].f0 = 9;
      b.finish(); HostSceneImage im; std::string e;
      if (build_host_image(im, &b.d, e, 0, 8, kLayoutTopLevels, true, kTwinBudgetBytes, 1) || e.find("out of range") == std::string::npos) return fail("object id out of range: " + e); }
    std::printf("ok\n");
    return 0;
}
