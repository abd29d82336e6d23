// Host-side unit test of the scene edits (aten_amd/csrc/host/scene_upload.hpp: pure host C++, compiled with hipcc for its headers
// only -- no HIP call is made, no GPU is needed).  For a small hand-made scene X and a list of edits, the host half of an edit call
// (edit_materials / edit_lights / edit_texture / edit_config on the SceneSource of X's upload) must leave what build_host_image
// gives for the edited description X': DevMaterial[], carpaint and toon byte for byte, any_alpha, material_set, rr_lookahead,
// nee_deferral and the textures' has-alpha flags field for field.  A refused edit leaves the state untouched.
// Prints "ok" or the first thing that is wrong (exit code 1).
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "../../aten_amd/csrc/host/scene_upload.hpp"
#include "../../include/aten_amd_scene.h"

using namespace atn;

static int fail(const std::string& what) { std::printf("FAILED: %s\n", what.c_str()); return 1; }

// The caller's side of a scene: the arrays and the description that points at them.
struct Scene {
    std::vector<atn_vec4> pos, nml;
    std::vector<atn_triangle_param> tris;
    std::vector<atn_object_param> objs;
    std::vector<atn_mat4> mtx;
    std::vector<atn_material_param> mats;
    std::vector<atn_light_param> lights, npr;
    std::vector<std::vector<atn_vec4>> texels;
    std::vector<atn_texture_desc> tex;
    std::vector<atn_bvh_node> blas, tlas;
    std::vector<atn_bvh_list> lists;
    atn_scene_desc d{};
    void point()        // the description at the arrays as they are now
    {
        for (size_t i = 0; i < tex.size(); i++) tex[i].texels = texels[i].data();
        d.objects = objs.data(); d.n_objects = (uint32_t)objs.size(); d.matrices = mtx.data(); d.n_matrices = (uint32_t)mtx.size();
        d.materials = mats.data(); d.n_materials = (uint32_t)mats.size(); d.lights = lights.data(); d.n_lights = (uint32_t)lights.size();
        d.triangles = tris.data(); d.n_triangles = (uint32_t)tris.size();
        d.vtx_pos = pos.data(); d.vtx_nml = nml.data(); d.n_vertices = (uint32_t)pos.size();
        d.bvh_lists = lists.data(); d.n_bvh_lists = (uint32_t)lists.size(); d.textures = tex.data(); d.n_textures = (uint32_t)tex.size();
        d.npr_target_lights = npr.data(); d.n_npr_target_lights = (uint32_t)npr.size();
    }
};

static atn_material_param material(int32_t type, float alpha = 1.0F, int32_t albedo = -1)
{
    atn_material_param m;
    std::memset(&m, 0, sizeof(m));
    m.baseColor = { 0.7F, 0.6F, 0.5F, alpha };
    m.type = type; m.albedoMap = albedo; m.normalMap = m.roughnessMap = -1;
    m.u.standard.ior = 1.5F; m.u.standard.roughness = 0.3F;
    m.toon.target_light_idx = -1; m.toon.remap_texture = -1;
    return m;
}

// four quads (one per material) under one instance, an area light on the instance and a directional light, one NPR target light,
// two 2 x 2 textures: [0] opaque (the albedo map of material 2), [1] opaque
static bool make_scene(Scene& s)
{
    for (int q = 0; q < 4; q++) {
        const float x = (float)q;
        const float c[4][2] = { { 0, 0 }, { 1, 0 }, { 1, 1 }, { 0, 1 } };
        for (auto& k : c) { s.pos.push_back({ x + k[0], 0.0F, k[1], k[0] }); s.nml.push_back({ 0.0F, 1.0F, 0.0F, k[1] }); }
        for (int k = 0; k < 2; k++) {
            atn_triangle_param t{};
            t.idx[0] = 4 * q; t.idx[1] = 4 * q + 1 + k; t.idx[2] = 4 * q + 2 + k;
            t.area = 0.5F; t.mtrlid = q; t.mesh_id = 0;
            s.tris.push_back(t);
        }
    }
    std::vector<uint32_t> ids(s.tris.size());
    for (size_t i = 0; i < ids.size(); i++) ids[i] = (uint32_t)i;
    atn_bvh_node* out = nullptr; uint32_t cnt = 0; float bmin[3], bmax[3];
    if (atns_build_blas(s.pos.data(), s.tris.data(), ids.data(), (uint32_t)ids.size(), &out, &cnt, bmin, bmax) != 0) return false;
    s.blas.assign(out, out + cnt); atns_free(out);
    atn_object_param poly{}; poly.type = ATN_OBJ_POLYGONS; poly.object_id = -1; poly.mtx_id = -1; poly.triangle_id = 0; poly.triangle_num = (int32_t)s.tris.size(); poly.light_id = -1;
    atn_object_param inst{}; inst.type = ATN_OBJ_INSTANCE; inst.object_id = 0; inst.mtx_id = 0; inst.triangle_id = -1; inst.light_id = 0;
    s.objs = { poly, inst };
    atn_mat4 id{};
    for (int a = 0; a < 4; a++) id.m[a][a] = 1.0F;
    s.mtx = { id, id };
    s.mats = { material(ATN_MTRL_DIFFUSE), material(ATN_MTRL_GGX), material(ATN_MTRL_DIFFUSE, 1.0F, 0), material(ATN_MTRL_SPECULAR) };
    for (size_t i = 0; i < s.mats.size(); i++) s.mats[i].id = (uint16_t)i;
    atn_light_param area{}; area.type = ATN_LIGHT_AREA; area.arealight_objid = 1; area.envmapidx = -1; area.intensity = 1.0F;
    atn_light_param dir{}; dir.type = ATN_LIGHT_DIRECTION; dir.attrib = ATN_LIGHT_ATTR_INFINITE | ATN_LIGHT_ATTR_SINGULAR; dir.arealight_objid = -1; dir.envmapidx = -1; dir.dir = { 0, -1, 0, 0 };
    s.lights = { area, dir };
    atn_light_param target{}; target.type = ATN_LIGHT_POINT; target.arealight_objid = -1; target.envmapidx = -1; target.pos = { 0, 2, 0, 1 };
    s.npr = { target };
    s.texels = { std::vector<atn_vec4>(4, atn_vec4{ 1.0F, 0.0F, 1.0F, 1.0F }), std::vector<atn_vec4>(4, atn_vec4{ 0.5F, 0.25F, 0.125F, 1.0F }) };
    s.tex = { { nullptr, 2, 2 }, { nullptr, 2, 2 } };
    const int32_t oid = 1, lid = 1, mid = 0;
    const float box[6] = { bmin[0], bmin[1], bmin[2], bmax[0], bmax[1], bmax[2] };
    if (atns_build_tlas(box, &oid, &lid, &mid, 1, &out, &cnt) != 0) return false;
    s.tlas.assign(out, out + cnt); atns_free(out);
    s.lists = { { s.tlas.data(), (uint32_t)s.tlas.size(), 0 }, { s.blas.data(), (uint32_t)s.blas.size(), 0 } };
    s.d.config.bvh_hit_min = -1.0F; s.d.config.bg.envmap_tex_idx = -1;
    for (int a = 0; a < 3; a++) { s.d.scene_bbox_min[a] = box[a]; s.d.scene_bbox_max[a] = box[3 + a]; }
    s.point();
    return true;
}

// What an edit has to get right, as the context holds it: the source and what is derived from it.
struct State {
    SceneSource src;
    MaterialState ms;
    int32_t nee_deferral = 0;
};

static bool from_upload(State& st, const Scene& s, std::string& err)
{
    HostSceneImage img;
    if (!build_host_image(img, &s.d, err, 0, 8, kLayoutTopLevels, true)) return false;
    st.src = img.source;
    st.ms.materials = img.materials; st.ms.carpaint = img.carpaint; st.ms.toon = img.toon;
    st.ms.any_alpha = img.params.any_alpha; st.ms.material_set = img.params.material_set; st.ms.rr_lookahead = img.params.rr_lookahead;
    st.nee_deferral = img.params.nee_deferral;
    return true;
}

template <class T>
static bool same_bytes(const std::vector<T>& a, const std::vector<T>& b)
{
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

static std::string differs(const State& a, const State& b)
{
    if (!same_bytes(a.ms.materials, b.ms.materials)) return "DevMaterial[]";
    if (!same_bytes(a.ms.carpaint, b.ms.carpaint)) return "carpaint";
    if (!same_bytes(a.ms.toon, b.ms.toon)) return "toon";
    if (a.ms.any_alpha != b.ms.any_alpha) return "any_alpha";
    if (a.ms.material_set != b.ms.material_set) return "material_set";
    if (a.ms.rr_lookahead != b.ms.rr_lookahead) return "rr_lookahead";
    if (a.nee_deferral != b.nee_deferral) return "nee_deferral";
    if (a.src.tex.size() != b.src.tex.size()) return "texture count";
    for (size_t i = 0; i < a.src.tex.size(); i++) if (a.src.tex[i].has_alpha != b.src.tex[i].has_alpha) return "texture has-alpha flag";
    if (!same_bytes(a.src.materials, b.src.materials) || !same_bytes(a.src.lights, b.src.lights) || !same_bytes(a.src.npr_lights, b.src.npr_lights)) return "source arrays";
    if (std::memcmp(&a.src.config, &b.src.config, sizeof(a.src.config)) != 0) return "source config";
    return "";
}

// the host half of the four entry points, on a State (the context's update_* do the same and then write the device)
static bool apply_materials(State& st, const atn_material_param* m, uint32_t n, uint32_t first, std::string& err)
{
    MaterialState ms;
    if (!edit_materials(st.src, m, n, first, ms, err)) return false;
    st.ms = ms;
    st.nee_deferral = nee_deferral_class(st.ms.material_set, st.src.lights.data(), (uint32_t)st.src.lights.size());
    return true;
}
static bool apply_lights(State& st, const atn_light_param* l, uint32_t n, uint32_t first, bool npr, std::string& err)
{
    if (!edit_lights(st.src, l, n, first, npr, err)) return false;
    st.nee_deferral = nee_deferral_class(st.ms.material_set, st.src.lights.data(), (uint32_t)st.src.lights.size());
    return true;
}
static bool apply_texture(State& st, int32_t texid, const atn_texture_desc& t, std::string& err)
{
    MaterialState ms;
    bool rederived = false;
    if (!edit_texture(st.src, texid, t, ms, rederived, err)) return false;
    if (rederived) st.ms = ms;
    return true;
}

int main()
{
    Scene x;
    if (!make_scene(x)) return fail("scene");
    std::string err;
    State a;
    if (!from_upload(a, x, err)) return fail("upload: " + err);
    if (a.ms.material_set != kMsCore || a.ms.any_alpha != 0 || a.ms.rr_lookahead != 1 || a.nee_deferral != 1) return fail("the start scene is core, opaque, look-ahead valid, deferral class 1");

    // One step: `change` edits the caller's arrays (X -> X'), `edit` makes the same change on the context's state.  Afterwards the
    // state must be what a fresh upload of X' gives.
    auto step = [&](const char* name, const std::function<void(Scene&)>& change, const std::function<bool(State&, const Scene&, std::string&)>& edit) -> std::string {
        change(x);
        x.point();
        std::string e;
        if (!edit(a, x, e)) return std::string(name) + ": the edit was refused: " + e;
        State b;
        if (!from_upload(b, x, e)) return std::string(name) + ": upload of the edited scene: " + e;
        const std::string d = differs(a, b);
        return d.empty() ? "" : std::string(name) + ": " + d + " differs from a fresh upload";
    };
    auto set_type = [&](const char* name, uint32_t i, int32_t type, int32_t want_set, int32_t want_rr) -> std::string {
        const std::string r = step(name, [&](Scene& s) { s.mats[i].type = type; },
                                   [&](State& st, const Scene& s, std::string& e) { return apply_materials(st, &s.mats[i], 1, i, e); });
        if (!r.empty()) return r;
        if (a.ms.material_set != want_set) return std::string(name) + ": material_set " + std::to_string(a.ms.material_set);
        if (a.ms.rr_lookahead != want_rr) return std::string(name) + ": rr_lookahead " + std::to_string(a.ms.rr_lookahead);
        return "";
    };
    std::string r;
    // ---- each material-set crossing, there and back (one material, a partial range)
    if (!(r = set_type("core -> Disney", 1, ATN_MTRL_DISNEY, kMsDisney, 1)).empty()) return fail(r);
    if (!(r = set_type("Disney -> core", 1, ATN_MTRL_GGX, kMsCore, 1)).empty()) return fail(r);
    if (!(r = set_type("core -> analytic (Refraction)", 3, ATN_MTRL_REFRACTION, kMsAnalytic, 1)).empty()) return fail(r);
    if (!(r = set_type("analytic -> core", 3, ATN_MTRL_SPECULAR, kMsCore, 1)).empty()) return fail(r);
    if (!(r = step("core -> CarPaint", [&](Scene& s) { s.mats[1].type = ATN_MTRL_CARPAINT; for (int k = 0; k < 16; k++) s.mats[1].u.carpaint[k] = 0.01F * (float)(k + 1); },
                   [&](State& st, const Scene& s, std::string& e) { return apply_materials(st, s.mats.data(), (uint32_t)s.mats.size(), 0, e); })).empty()) return fail(r);
    if (a.ms.material_set != kMsCarPaint || a.ms.rr_lookahead != 0 || a.nee_deferral != 0 || a.ms.carpaint[4 * 1 + 3].w != 0.16F) return fail("CarPaint: set, look-ahead, deferral class or side table");
    if (!(r = step("CarPaint -> core", [&](Scene& s) { s.mats[1] = material(ATN_MTRL_GGX); s.mats[1].id = 1; },
                   [&](State& st, const Scene& s, std::string& e) { return apply_materials(st, s.mats.data(), (uint32_t)s.mats.size(), 0, e); })).empty()) return fail(r);
    if (!(r = step("core -> Toon", [&](Scene& s) { s.mats[0].type = ATN_MTRL_TOON; s.mats[0].toon.target_light_idx = 0; s.mats[0].toon.toon_type = ATN_MTRL_DIFFUSE; },
                   [&](State& st, const Scene& s, std::string& e) { return apply_materials(st, &s.mats[0], 1, 0, e); })).empty()) return fail(r);
    if (a.ms.material_set != kMsToon || a.ms.rr_lookahead != 0 || a.ms.toon[0].target_light_idx != 0) return fail("Toon: set, look-ahead or side table");
    if (!(r = step("Toon -> core", [&](Scene& s) { s.mats[0] = material(ATN_MTRL_DIFFUSE); },
                   [&](State& st, const Scene& s, std::string& e) { return apply_materials(st, &s.mats[0], 1, 0, e); })).empty()) return fail(r);
    if (a.ms.material_set != kMsCore || a.ms.rr_lookahead != 1 || a.nee_deferral != 1) return fail("back in the core set");
    // a singular attribute switches the look-ahead off without leaving the set
    if (!(r = step("Specular + SINGULAR", [&](Scene& s) { s.mats[3].attrib = ATN_MTRL_ATTR_SINGULAR; },
                   [&](State& st, const Scene& s, std::string& e) { return apply_materials(st, &s.mats[3], 1, 3, e); })).empty()) return fail(r);
    if (a.ms.rr_lookahead != 0 || a.ms.material_set != kMsCore) return fail("a singular material switches the look-ahead off");
    if (!(r = step("Specular - SINGULAR", [&](Scene& s) { s.mats[3].attrib = 0; },
                   [&](State& st, const Scene& s, std::string& e) { return apply_materials(st, &s.mats[3], 1, 3, e); })).empty()) return fail(r);

    // ---- alpha via baseColor.w
    if (!(r = step("baseColor.w = 0.4", [&](Scene& s) { s.mats[1].baseColor.w = 0.4F; },
                   [&](State& st, const Scene& s, std::string& e) { return apply_materials(st, &s.mats[1], 1, 1, e); })).empty()) return fail(r);
    if (a.ms.any_alpha != 1 || !(a.ms.materials[1].attrib & kAttrMaybeAlpha) || (a.ms.materials[0].attrib & kAttrMaybeAlpha)) return fail("baseColor.w < 1: kAttrMaybeAlpha / any_alpha");
    if (!(r = step("baseColor.w = 1", [&](Scene& s) { s.mats[1].baseColor.w = 1.0F; },
                   [&](State& st, const Scene& s, std::string& e) { return apply_materials(st, &s.mats[1], 1, 1, e); })).empty()) return fail(r);
    if (a.ms.any_alpha != 0) return fail("opaque again");
    // ---- alpha via the albedo texture: texture 0 is material 2's albedo map
    if (!(r = step("albedo texel alpha 0.5", [&](Scene& s) { s.texels[0][3].w = 0.5F; },
                   [&](State& st, const Scene& s, std::string& e) { return apply_texture(st, 0, s.tex[0], e); })).empty()) return fail(r);
    if (a.ms.any_alpha != 1 || !(a.ms.materials[2].attrib & kAttrMaybeAlpha) || !a.src.tex[0].has_alpha) return fail("texture alpha: kAttrMaybeAlpha of the material that names it");
    // (a texture nobody names as albedo map: the flag follows, the materials do not)
    if (!(r = step("unused texture alpha", [&](Scene& s) { s.texels[1][0].w = 0.0F; },
                   [&](State& st, const Scene& s, std::string& e) { return apply_texture(st, 1, s.tex[1], e); })).empty()) return fail(r);
    if (!(r = step("material 1 takes texture 1 as albedo map", [&](Scene& s) { s.mats[1].albedoMap = 1; },
                   [&](State& st, const Scene& s, std::string& e) { return apply_materials(st, &s.mats[1], 1, 1, e); })).empty()) return fail(r);
    if (!(a.ms.materials[1].attrib & kAttrMaybeAlpha)) return fail("a material edit sees the texture's alpha flag");
    if (!(r = step("textures opaque again", [&](Scene& s) { s.texels[0][3].w = 1.0F; s.texels[1][0].w = 1.0F; },
                   [&](State& st, const Scene& s, std::string& e) { return apply_texture(st, 0, s.tex[0], e) && apply_texture(st, 1, s.tex[1], e); })).empty()) return fail(r);
    if (a.ms.any_alpha != 0) return fail("opaque textures: any_alpha");
    // ---- stencil type 2 (and 1)
    if (!(r = step("stencil_type 2", [&](Scene& s) { s.mats[0].stencil_type = 2; s.mats[3].stencil_type = 1; },
                   [&](State& st, const Scene& s, std::string& e) { return apply_materials(st, s.mats.data(), (uint32_t)s.mats.size(), 0, e); })).empty()) return fail(r);
    if (a.ms.any_alpha != 1 || !(a.ms.materials[0].attrib & kAttrStencilStencil) || !(a.ms.materials[3].attrib & kAttrStencilAlways)) return fail("stencil bits / any_alpha");
    if (!(r = step("stencil_type 0", [&](Scene& s) { s.mats[0].stencil_type = 0; s.mats[3].stencil_type = 0; },
                   [&](State& st, const Scene& s, std::string& e) { return apply_materials(st, s.mats.data(), (uint32_t)s.mats.size(), 0, e); })).empty()) return fail(r);

    // ---- a light type change: the area light becomes a directional one -> every light infinite -> deferral class 3, and back
    if (!(r = step("area -> directional", [&](Scene& s) { s.lights[0] = s.lights[1]; s.lights[0].dir = { 1, 0, 0, 0 }; },
                   [&](State& st, const Scene& s, std::string& e) { return apply_lights(st, &s.lights[0], 1, 0, false, e); })).empty()) return fail(r);
    if (a.nee_deferral != 3) return fail("all lights infinite: deferral class 3");
    if (!(r = step("directional -> point", [&](Scene& s) { s.lights[1].type = ATN_LIGHT_POINT; s.lights[1].attrib = ATN_LIGHT_ATTR_SINGULAR; },
                   [&](State& st, const Scene& s, std::string& e) { return apply_lights(st, s.lights.data(), 2, 0, false, e); })).empty()) return fail(r);
    if (a.nee_deferral != 1) return fail("a finite light: deferral class 1");
    if (!(r = step("NPR target light moved", [&](Scene& s) { s.npr[0].pos = { 3, 1, 2, 1 }; },
                   [&](State& st, const Scene& s, std::string& e) { return apply_lights(st, s.npr.data(), 1, 0, true, e); })).empty()) return fail(r);
    // ---- the config
    if (!(r = step("config", [&](Scene& s) { s.d.config.enable_alpha_blending = 1; s.d.config.bg.envmap_tex_idx = 1; s.d.config.bg.enable_env_map = 1; s.d.config.bg.multiplyer = 2.0F; },
                   [&](State& st, const Scene& s, std::string& e) { return edit_config(st.src, s.d.config, e); })).empty()) return fail(r);

    // ---- refused edits leave the state untouched, and the upload refuses the same content with the same message
    auto refused = [&](const char* name, const std::function<bool(State&, std::string&)>& edit, const std::function<void(Scene&)>& change, const char* message) -> std::string {
        const State before = a;
        std::string e;
        if (edit(a, e)) return std::string(name) + ": not refused";
        if (e != message) return std::string(name) + ": message '" + e + "'";
        if (!differs(a, before).empty()) return std::string(name) + ": a refused edit changed " + differs(a, before);
        Scene y = x;
        change(y);
        y.point();
        State b; std::string ue;
        if (from_upload(b, y, ue)) return std::string(name) + ": the upload accepts what the edit refuses";
        if (ue != e) return std::string(name) + ": the upload says '" + ue + "'";
        return "";
    };
    atn_material_param bad_map = x.mats[1]; bad_map.albedoMap = 2;
    if (!(r = refused("albedoMap out of range", [&](State& st, std::string& e) { return apply_materials(st, &bad_map, 1, 1, e); },
                      [&](Scene& s) { s.mats[1] = bad_map; }, "material texture index out of range")).empty()) return fail(r);
    atn_material_param bad_toon = x.mats[0]; bad_toon.type = ATN_MTRL_TOON; bad_toon.toon.target_light_idx = 1;
    std::vector<atn_material_param> two = { bad_toon, x.mats[1] };
    two[1].baseColor.w = 0.25F;         // (a valid change in the same call must not get through either)
    if (!(r = refused("toon target light out of range", [&](State& st, std::string& e) { return apply_materials(st, two.data(), 2, 0, e); },
                      [&](Scene& s) { s.mats[0] = two[0]; s.mats[1] = two[1]; }, "toon material's target light index out of range")).empty()) return fail(r);
    atn_light_param bad_light = x.lights[0]; bad_light.type = ATN_LIGHT_AREA; bad_light.arealight_objid = 2;
    if (!(r = refused("light object out of range", [&](State& st, std::string& e) { return apply_lights(st, &bad_light, 1, 0, false, e); },
                      [&](Scene& s) { s.lights[0] = bad_light; }, "light refers to an object id out of range")).empty()) return fail(r);
    atn_light_param bad_ibl = x.lights[1]; bad_ibl.type = ATN_LIGHT_IBL; bad_ibl.envmapidx = 2;
    if (!(r = refused("IBL envmapidx out of range", [&](State& st, std::string& e) { return apply_lights(st, &bad_ibl, 1, 1, false, e); },
                      [&](Scene& s) { s.lights[1] = bad_ibl; }, "IBL light's environment map index out of range")).empty()) return fail(r);
    atn_scene_rendering_config bad_cfg = x.d.config; bad_cfg.bg.envmap_tex_idx = 2;
    if (!(r = refused("config envmap out of range", [&](State& st, std::string& e) { return edit_config(st.src, bad_cfg, e); },
                      [&](Scene& s) { s.d.config = bad_cfg; }, "the config's environment map texture index out of range")).empty()) return fail(r);
    {   // a texture of another size: refused by the edit (an upload takes any size: there is nothing to compare with)
        const State before = a;
        std::vector<atn_vec4> big(8, atn_vec4{ 0, 0, 0, 0.5F });
        const atn_texture_desc t{ big.data(), 4, 2 };
        std::string e;
        if (apply_texture(a, 0, t, e) || e != "a texture update keeps the texture's size" || !differs(a, before).empty()) return fail("a texture of another size");
    }
    // the edits went through the whole list: once more against a fresh upload
    State b;
    if (!from_upload(b, x, err) || !differs(a, b).empty()) return fail("the state after all edits: " + differs(a, b));
    std::printf("ok\n");
    return 0;
}
