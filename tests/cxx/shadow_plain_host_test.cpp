// Host-side unit test of DevScene::shadow_plain's decision (aten_amd/csrc/host/scene_upload.hpp: shadow_plain_class -- pure host C++,
// compiled with hipcc for its headers only; no HIP call is made, no GPU is needed).  The flag says "every light is infinite and none is
// an area light with an object": then a shadow ray reaches its light iff it hits nothing and the shadow job reads no light record
// (device/kernels.hpp, ShadowJob).  Checked for the light lists a scene can have, and that the host half of a light edit
// (edit_lights on the SceneSource, then the decision again -- what atn_update_lights does) gives what an upload of the edited list gives.
// Prints "ok" or the first thing that is wrong (exit code 1).
#include <cstdio>
#include <string>
#include <vector>

#include "../../aten_amd/csrc/host/scene_upload.hpp"

using namespace atn;

static int fail(const std::string& what) { std::printf("FAILED: %s\n", what.c_str()); return 1; }

static atn_light_param light(int32_t type, uint32_t attrib, int32_t objid = -1, int32_t envmap = -1)
{
    atn_light_param l{};
    l.type = type; l.attrib = attrib; l.arealight_objid = objid; l.envmapidx = envmap; l.intensity = 1.0F; l.scale = 1.0F;
    return l;
}

static int32_t decide(const std::vector<atn_light_param>& l) { return shadow_plain_class(l.data(), (uint32_t)l.size()); }

int main()
{
    const atn_light_param ibl = light(ATN_LIGHT_IBL, ATN_LIGHT_ATTR_INFINITE | ATN_LIGHT_ATTR_IBL, -1, 0);
    const atn_light_param directional = light(ATN_LIGHT_DIRECTION, ATN_LIGHT_ATTR_INFINITE | ATN_LIGHT_ATTR_SINGULAR);
    const atn_light_param point = light(ATN_LIGHT_POINT, ATN_LIGHT_ATTR_SINGULAR);
    const atn_light_param spot = light(ATN_LIGHT_SPOT, ATN_LIGHT_ATTR_SINGULAR);
    const atn_light_param lamp = light(ATN_LIGHT_AREA, 0, 1);                 // an area light on object 1
    const atn_light_param bare_area = light(ATN_LIGHT_AREA, 0, -1);           // an area light without an object: not infinite
    const atn_light_param infinite_lamp = light(ATN_LIGHT_AREA, ATN_LIGHT_ATTR_INFINITE, 1);    // (the attribute does not take the object away)
    const atn_light_param infinite_bare_area = light(ATN_LIGHT_AREA, ATN_LIGHT_ATTR_INFINITE, -1);

    struct Case { const char* name; std::vector<atn_light_param> lights; int32_t want; };
    const Case cases[] = {
        { "no light", {}, 0 },                                   // no shadow ray is cast: the flag stays off
        { "IBL only", { ibl }, 1 },
        { "directional only", { directional }, 1 },
        { "IBL + directional", { ibl, directional }, 1 },
        { "IBL + point", { ibl, point }, 0 },
        { "point + IBL", { point, ibl }, 0 },
        { "spot only", { spot }, 0 },
        { "area light with an object", { lamp }, 0 },
        { "directional + area light with an object", { directional, lamp }, 0 },
        { "area light without an object", { bare_area }, 0 },
        { "infinite area light with an object", { ibl, infinite_lamp }, 0 },
        { "infinite area light without an object", { ibl, infinite_bare_area }, 1 },
    };
    for (const Case& c : cases)
        if (decide(c.lights) != c.want) return fail(std::string(c.name) + ": shadow_plain " + std::to_string(decide(c.lights)));
    if (shadow_plain_class(nullptr, 3) != 0) return fail("a null light array");

    // the flag implies the deferral policy's "every light is infinite" (nee_deferral_class bit 1) wherever the material set qualifies
    for (const Case& c : cases)
        if (c.want && nee_deferral_class(kMsCore, c.lights.data(), (uint32_t)c.lights.size()) != 3) return fail(std::string(c.name) + ": plain without deferral class 3");

    // ---- an edit decides again: the host half of atn_update_lights on a context's SceneSource
    SceneSource src;
    src.lights = { ibl, directional };
    src.n_objects = 2;
    src.tex.resize(1);
    auto edit = [&](const char* name, const std::vector<atn_light_param>& l, uint32_t first, int32_t want) -> std::string {
        std::string err;
        if (!edit_lights(src, l.data(), (uint32_t)l.size(), first, false, err)) return std::string(name) + ": refused: " + err;
        const int32_t got = shadow_plain_class(src.lights.data(), (uint32_t)src.lights.size());
        if (got != want) return std::string(name) + ": shadow_plain " + std::to_string(got) + " after the edit";
        // what an upload of the edited list decides (build_host_image calls the same function on the caller's array)
        const std::vector<atn_light_param> uploaded = src.lights;
        if (decide(uploaded) != got) return std::string(name) + ": differs from an upload";
        return "";
    };
    std::string r;
    if (decide(src.lights) != 1) return fail("IBL + directional before any edit");
    if (!(r = edit("directional -> point", { point }, 1, 0)).empty()) return fail(r);
    if (!(r = edit("point -> directional", { directional }, 1, 1)).empty()) return fail(r);
    if (!(r = edit("IBL -> lamp", { lamp }, 0, 0)).empty()) return fail(r);
    if (!(r = edit("both at once: IBL + directional", { ibl, directional }, 0, 1)).empty()) return fail(r);
    if (!(r = edit("an empty range changes nothing", {}, 0, 1)).empty()) return fail(r);
    {   // a refused edit (object id out of range) leaves the lights, and with them the flag, as they were
        const atn_light_param bad = light(ATN_LIGHT_AREA, 0, 7);
        std::string err;
        if (edit_lights(src, &bad, 1, 0, false, err)) return fail("an out-of-range object id was accepted");
        if (decide(src.lights) != 1) return fail("a refused edit changed the flag");
    }
    std::printf("ok\n");
    return 0;
}
