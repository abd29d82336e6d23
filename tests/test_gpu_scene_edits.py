"""Scene edits (atn_update_materials / _lights / _texture / _rendering_config, docs/SCENE_EDITS.md) against a fresh upload.

Context A uploads X and edits it to X'; context B uploads X'.  Both render the same frames with the same seeds, and every film
comparison is tobytes() equality: nothing here has a tolerance.  An edit resets nothing, so both sides call the renderer's reset
before they render.  Frames are 64 x 48, depth 5, roulette from 3, three progressive frames unless a test says otherwise."""
import ctypes as C
import os

import numpy as np
import pytest

from aten_amd import layout as L
from aten_amd.renderer import AtenAmdError, MultiGpuPathTracing, PathTracing
from aten_amd.scene import scenedefs
from aten_amd.scene.builder import SceneBuilder
from aten_amd.scene.camera import create_camera

pytestmark = pytest.mark.gpu

W, H, DEPTH, RR, FRAMES = 64, 48, 5, 3, 3
INVALID_ARG, NO_SCENE, UNSUPPORTED = -1, -4, -5


def new_context(fs, cam, w=W, h=H, setup=None):
    r = PathTracing(0)
    try:
        if setup:
            setup(r)
        r.UpdateSceneData(fs)
        r.updateCamera(create_camera(cam["pos"], cam["at"], cam["vfov"], w, h))
        r.initSampler(w, h, 0)
    except Exception:
        r.close()
        raise
    return r


def film(r, renderer="render", w=W, h=H, frames=FRAMES, first=0):
    """The film after `frames` progressive frames of one renderer, from its reset."""
    {"render": r.reset, "svgf_render": r.svgf_reset, "restir_render": r.restir_reset, "npr_render": r.npr_reset,
     "volume_render": r.volume_reset, "ao_render": r.ao_reset}[renderer]()
    if renderer in ("svgf_render", "restir_render"):
        r.reset()                   # (their resets drop the histories; the progressive film is atn_reset's)
    out = None
    for k in range(first, first + frames):
        if renderer == "ao_render":
            out = r.ao_render(w, h, frame=k, break_on_terminate=False)
        elif renderer == "restir_render":
            out = r.restir_render(w, h, DEPTH, RR, frame=k, compute_motion=True)
        elif renderer == "svgf_render":
            out = r.svgf_render(w, h, DEPTH, RR, frame=k, compute_motion=True)
        else:
            out = getattr(r, renderer)(w, h, DEPTH, RR, frame=k)
    return out.tobytes()


def material(mtype, base_color, index, **kw):
    """A material record as SceneBuilder writes it, for slot `index` of a scene's material array."""
    b = SceneBuilder()
    if mtype == L.MTRL_CARPAINT:
        b.add_carpaint_material("m", base_color, **kw)
    elif mtype in (L.MTRL_TOON, L.MTRL_STYLIZED):
        b.add_toon_material("m", base_color, stylized=mtype == L.MTRL_STYLIZED, **kw)
    else:
        b.add_material("m", mtype, base_color, **kw)
    m = b.materials[0][1].copy()
    m["id"] = index
    return m


def npr_target_lights(fs):
    """The scene's NPR target lights as a numpy view of the array the description points at."""
    n = int(fs.desc.n_npr_target_lights)
    buf = (C.c_char * (n * L.LIGHT_PARAM.itemsize)).from_address(fs.desc.npr_target_lights)
    return np.frombuffer(buf, L.LIGHT_PARAM)


def lampless_room(toon_target=False):
    """The Cornell box's geometry without its lamp under a point light: Lambert surfaces and a GGX floor -- the core material set, no
    emissive material, so the roulette look-ahead and the deferred NEE both qualify."""
    b = SceneBuilder()

    def create_mtrl(name, mtype, clr, albedo, nml):
        if name == "floor":
            return b.add_material(name, L.MTRL_GGX, clr, roughness=0.2, ior=0.01)
        return b.add_material(name, L.MTRL_DIFFUSE, clr)

    objs = b.load_obj(os.path.join(scenedefs.ASSETS, "cornellbox", "orig.obj"), create_mtrl=create_mtrl, separate_objs=True, normal_on_the_fly=True)
    for o in objs:
        if b.objects[o]["name"] != "light":
            b.create_instance(o)
    b.add_point_light((0.3, 1.6, 0.4), (1.0, 0.9, 0.8), 3.0)
    if toon_target:
        b.add_npr_target_light(b.lights[0])
    b.set_background((0.3, 0.4, 0.5))
    return b.build(), dict(pos=(0.0, 1.0, 3.0), at=(0.0, 1.0, 0.0), vfov=45.0)


class Pair:
    """A (edited) and B (fresh upload of what A was edited to), compared after every step."""

    def __init__(self, fs, cam, setup=None, w=W, h=H):
        self.fs, self.cam, self.setup, self.w, self.h = fs, cam, setup, w, h
        self.a = new_context(fs, cam, w, h, setup)

    def step(self, change, apply, renderers=("render",), probes=(), what=""):
        """`change` edits the scene's arrays (X -> X'), `apply` hands the edit to A; then B uploads X'."""
        change()
        apply(self.a)
        b = new_context(self.fs, self.cam, self.w, self.h, self.setup)
        try:
            for p in probes:
                assert p(self.a) == p(b), (what, p(self.a), p(b))
            for rn in renderers:
                assert film(self.a, rn, self.w, self.h) == film(b, rn, self.w, self.h), (what, rn)
        finally:
            b.close()

    def close(self):
        self.a.close()


# ---- 1. materials within the core set -----------------------------------------------------------------------------------------------
def test_material_edits_within_the_core_set():
    fs, cam = scenedefs.cornell_box()
    mats, names = fs.arrays["materials"], fs.names["materials"]
    wall, box = names.index("leftWall"), names.index("tallBox")
    assert 0 < wall and 0 < box
    p = Pair(fs, cam)
    try:
        before = film(p.a)
        kept = p.a.planar_area_lights()

        def recolour():
            mats["baseColor"][wall] = (0.1, 0.8, 0.3, 1.0)
        p.step(recolour, lambda r: r.updateMaterial(fs, first=wall, n=1), what="partial range")
        assert film(p.a) != before                                     # (the edit is visible)

        def ggx():
            mats[box] = material(L.MTRL_GGX, (0.8, 0.7, 0.2), box, roughness=0.35, ior=0.02)
        p.step(ggx, lambda r: r.updateMaterial(fs), what="whole array")
        assert p.a.planar_area_lights() == kept
        # nothing is reset by an edit: the film on the device is still the one rendered last
        held = p.a.download_film().tobytes()
        p.a.updateMaterial(fs, first=box, n=1)
        assert p.a.download_film().tobytes() == held
    finally:
        p.close()


# ---- 2. material-set crossings ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["rr_lookahead", "nee_deferral"])
def test_material_set_crossings(mode):
    fs, cam = lampless_room(toon_target=True)
    mats, names = fs.arrays["materials"], fs.names["materials"]
    box, tall = names.index("shortBox"), names.index("tallBox")
    core = mats[box].copy()
    setup = (lambda r: r.set_rr_lookahead(1)) if mode == "rr_lookahead" else (lambda r: r.set_nee_deferral(1))
    probes = (lambda r: r.rr_lookahead_active(), lambda r: r.nee_deferral_active())
    p = Pair(fs, cam, setup)
    try:
        assert p.a.rr_lookahead_active() and (mode != "nee_deferral" or p.a.nee_deferral_active())

        def put(m):
            def change():
                mats[box] = m
            return change
        edit = lambda r: r.updateMaterial(fs, first=box, n=1)
        p.step(put(material(L.MTRL_DISNEY, (0.7, 0.6, 0.5), box, roughness=0.35, metallic=0.3, specular=0.6, clearcoat=0.4)), edit, probes=probes, what="core -> Disney")
        p.step(put(core), edit, probes=probes, what="Disney -> core")
        p.step(put(material(L.MTRL_CARPAINT, (1.0, 1.0, 1.0), box, diffuse_color=(0.1, 0.3, 0.8), flake_size=0.4)), edit, probes=probes, what="core -> CarPaint")
        assert not p.a.rr_lookahead_active() and not p.a.nee_deferral_active()
        p.step(put(core), edit, probes=probes, what="CarPaint -> core")
        assert p.a.rr_lookahead_active()
        p.step(put(material(L.MTRL_REFRACTION, (0.9, 0.9, 0.9), box, ior=1.5)), edit, probes=probes, what="core -> Refraction")
        assert not p.a.rr_lookahead_active()                            # a singular material: the look-ahead is off
        p.step(put(core), edit, probes=probes, what="Refraction -> core")
        assert p.a.rr_lookahead_active()

        # Toon: ReSTIR refuses the edited scene exactly as it refuses the uploaded one
        def toon():
            mats[tall] = material(L.MTRL_TOON, (0.9, 0.5, 0.4), tall, target_light_idx=0)
        toon()
        p.a.updateMaterial(fs)
        b = new_context(fs, cam, setup=setup)
        try:
            said = []
            for r in (p.a, b):
                with pytest.raises(AtenAmdError, match=r"status -5") as e:
                    r.restir_render(W, H, DEPTH, RR)
                said.append(str(e.value))
            assert said[0] == said[1] and "toon" in said[0]
            assert film(p.a) == film(b)
        finally:
            b.close()
    finally:
        p.close()


# ---- 3. alpha -----------------------------------------------------------------------------------------------------------------------
def test_alpha_through_base_color():
    """The scene of test_shadow_rays_through_alpha_surfaces_with_alpha_blending, starting opaque: a box's alpha goes to 0.4
    (any_alpha 0 -> 1: shadow rays restart behind it) and back to 1."""
    fs, cam = scenedefs.cornell_box_variant(lights="point")
    fs.desc.config.enable_alpha_blending = 1
    mats, names = fs.arrays["materials"], fs.names["materials"]
    pane = names.index("shortBox")
    p = Pair(fs, cam)
    try:
        opaque = film(p.a)

        def alpha(a):
            def change():
                mats["baseColor"][pane][3] = a
            return change
        p.step(alpha(0.4), lambda r: r.updateMaterial(fs, first=pane, n=1), what="alpha 0.4")
        assert film(p.a) != opaque
        p.step(alpha(1.0), lambda r: r.updateMaterial(fs, first=pane, n=1), what="alpha 1")
        assert film(p.a) == opaque
    finally:
        p.close()


# ---- 4. lights ----------------------------------------------------------------------------------------------------------------------
def test_light_edits():
    fs, cam = scenedefs.cornell_box_variant(lights="mixed")
    lights = fs.arrays["lights"]
    kind = [int(t) for t in lights["type"]]
    area, point, spot, direc = (kind.index(t) for t in (L.LIGHT_AREA, L.LIGHT_POINT, L.LIGHT_SPOT, L.LIGHT_DIRECTION))
    p = Pair(fs, cam)
    try:
        planar = p.a.planar_area_lights()
        assert planar == 1
        probe = (lambda r: r.nee_deferral_active(),)

        def move_point():
            lights["pos"][point] = (-0.4, 1.2, 0.7, 1.0)
        p.step(move_point, lambda r: r.updateLight(fs, first=point, n=1), what="point moved")

        def angles():
            lights["innerAngle"][spot], lights["outerAngle"][spot] = np.radians(10.0), np.radians(35.0)
            d = np.array([0.5, -0.7, -0.5], np.float32)
            d /= np.linalg.norm(d)
            lights["dir"][direc] = (d[0], d[1], d[2], 0.0)
        p.step(angles, lambda r: r.updateLight(fs), what="spot angles, directional direction")
        assert p.a.planar_area_lights() == planar                       # (the area light came back with type and object unchanged)

        def intensity():
            lights["intensity"][area] = 60.0
        p.step(intensity, lambda r: r.updateLight(fs, first=area, n=1), what="area intensity")
        assert p.a.planar_area_lights() == planar

        def area_to_point():
            l = lights[point].copy()
            l["pos"] = (0.0, 1.9, 0.0, 1.0)
            lights[area] = l
        p.step(area_to_point, lambda r: r.updateLight(fs, first=area, n=1), what="area -> point")
        assert p.a.planar_area_lights() == planar - 1

        # under the deferral policy (mode 2): the directional light becomes a point light
        p.setup = lambda r: r.set_nee_deferral(2)
        p.a.set_nee_deferral(2)

        def directional_to_point():
            lights[direc] = lights[point]
            lights["pos"][direc] = (0.5, 1.0, 0.9, 1.0)
        p.step(directional_to_point, lambda r: r.updateLight(fs, first=direc, n=1), probes=probe, what="directional -> point, mode 2")
    finally:
        p.close()


def test_light_edit_decides_the_deferral_policy():
    """Mode 2 defers only where every light is infinite: a directional light that becomes a point light ends that."""
    fs, cam = scenedefs.cornell_box_variant(lights="directional")
    lights = fs.arrays["lights"]
    p = Pair(fs, cam, setup=lambda r: r.set_nee_deferral(2))
    try:
        assert p.a.nee_deferral_active()

        def to_point():
            lights["type"][0] = L.LIGHT_POINT
            lights["attrib"][0] = L.LATTR_SINGULAR
            lights["pos"][0] = (0.3, 1.6, 0.4, 1.0)
        p.step(to_point, lambda r: r.updateLight(fs), probes=(lambda r: r.nee_deferral_active(),), what="directional -> point")
        assert not p.a.nee_deferral_active()
    finally:
        p.close()


# ---- 5. NPR target lights -----------------------------------------------------------------------------------------------------------
def test_npr_target_light_edit():
    fs, cam = scenedefs.with_feature_lines(scenedefs.toon_room(stylized_shadow=("tallBox", "floor")))
    target = npr_target_lights(fs)
    p = Pair(fs, cam)
    try:
        def move():
            target["pos"][0] = (-0.5, 1.4, 0.9, 1.0)
        p.step(move, lambda r: r.updateLight(fs, npr_target=True), renderers=("render", "npr_render"), what="target moved")

        def move_again():
            target["pos"][0] = (0.6, 1.1, 1.0, 1.0)
        p.setup = lambda r: r.set_npr_shadow(1)
        p.a.set_npr_shadow(1)
        p.step(move_again, lambda r: r.updateLight(fs, npr_target=True, first=0, n=1), renderers=("render", "npr_render"), what="target moved, shadow pre-pass")
    finally:
        p.close()


# ---- 6. textures --------------------------------------------------------------------------------------------------------------------
def test_toon_ramp_repainted():
    fs, cam = scenedefs.toon_room()
    ramp = fs.names["textures"].index("ramp4")
    p = Pair(fs, cam)
    try:
        def repaint():
            fs.arrays["textures"][ramp][...] = scenedefs.toon_ramp((0.05, 0.3, 0.55, 0.9), tint=(1.0, 0.7, 0.9))
        p.step(repaint, lambda r: r.UpdateTexture(fs, ramp), what="toon ramp")
    finally:
        p.close()


def _textured_room():
    """The Cornell box's geometry without its lamp under a point light, with an 8-bit-exact albedo texture (k / 255) on the back wall
    and on the short box, which floats above the floor (its shadow is in view), alpha blending on."""
    b = SceneBuilder()
    rng = np.random.default_rng(11)
    tex = (rng.integers(0, 256, (16, 24, 4)).astype(np.float32) / np.float32(255.0)).astype(np.float32)
    tex[..., 3] = 1.0
    tid = b.add_texture("albedo8", tex)

    def create_mtrl(name, mtype, clr, albedo, nml):
        return b.add_material(name, L.MTRL_DIFFUSE, clr, albedo_map=tid if name in ("backWall", "shortBox") else -1)

    objs = b.load_obj(os.path.join(scenedefs.ASSETS, "cornellbox", "orig.obj"), create_mtrl=create_mtrl, separate_objs=True, normal_on_the_fly=True)
    for o in objs:
        n = b.objects[o]["name"]
        if n != "light":
            b.create_instance(o, np.array([[1, 0, 0, -0.2], [0, 1, 0, 0.25], [0, 0, 1, 0.05], [0, 0, 0, 1]], np.float32) if n == "shortBox" else None)
    b.add_point_light((0.3, 1.6, 0.4), (1.0, 0.9, 0.8), 40.0)
    b.config.enable_alpha_blending = 1
    b.set_background((0.02, 0.03, 0.05))
    return b.build(), dict(pos=(0.0, 1.0, 3.0), at=(0.0, 1.0, 0.0), vfov=45.0), tid


def test_texture_storage_and_alpha():
    """A texture stored as RGBA8 receives values that are not k / 255, then texels with alpha 0.5: every lookup returns exactly
    the floats handed in (bit-equal to a fresh upload, point and bilinear), and the has-alpha flag reaches the materials."""
    fs, cam, tid = _textured_room()
    tex = fs.arrays["textures"][tid]
    rng = np.random.default_rng(5)
    uv = rng.random((4096, 2)).astype(np.float32)
    uv[:64] = rng.choice(np.array([0.0, 1.0, 0.5, 1e-7, 0.9999999], np.float32), (64, 2))

    def lookups(r):
        out = []
        for bil in (False, True):
            r.set_sampling_options(tex_bilinear=bil)
            out.append(r.sample_texture(tid, uv).tobytes())
        r.set_sampling_options()
        return out

    p = Pair(fs, cam)
    try:
        def not_8bit():
            tex[..., :3] = rng.random(tex.shape[:2] + (3,)).astype(np.float32) * np.float32(1.7)
        p.step(not_8bit, lambda r: r.UpdateTexture(fs, tid), probes=(lookups,), what="values that are not k / 255")
        got = p.a.sample_texture(tid, np.array([[0.0, 0.0]], np.float32))
        assert got.tobytes() == tex[0, 0].tobytes()                     # exactly the floats handed in
        opaque = film(p.a)

        def volume_answer(r):
            try:
                r.volume_render(W, H, DEPTH, RR)
            except AtenAmdError as e:
                return str(e)
            return "rendered"
        assert volume_answer(p.a) == "rendered"

        def half_alpha():
            tex[..., 3] = 0.5
        p.step(half_alpha, lambda r: r.UpdateTexture(fs, tid), probes=(lookups, volume_answer), what="alpha 0.5 texels")
        assert film(p.a) != opaque                                      # shadow rays now pass through the short box
        assert "alpha" in volume_answer(p.a)                            # the flag reached the materials: volume frames refuse

        def eight_bit_again():
            tex[...] = (rng.integers(0, 256, tex.shape).astype(np.float32) / np.float32(255.0)).astype(np.float32)
        p.step(eight_bit_again, lambda r: r.UpdateTexture(fs, tid), probes=(lookups, volume_answer), what="8-bit content into float storage")
    finally:
        p.close()


def _env_sponza():
    """sponza_lod without its image textures under a 64 x 32 environment map, with a second map of the same size uploaded beside it."""
    env = scenedefs.synthetic_envmap(64, 32)
    other = np.ascontiguousarray(np.roll(env, 20, axis=1)[::-1] * np.float32(0.5))
    other[..., 3] = 1.0
    ids = {}

    def add(b, lo, hi, cam):
        ids["env"] = b.add_texture("env", env)
        ids["other"] = b.add_texture("other", other)
        b.add_ibl(ids["env"], avg_illum=scenedefs.envmap_avg_illum(env))
    fs, cam = scenedefs.sponza_lod(ibl=False, textures=False, add_lights=add)
    return fs, cam, ids, other


@pytest.mark.parametrize("importance", [False, True])
def test_environment_map_repainted(importance):
    fs, cam, ids, other = _env_sponza()
    tex = fs.arrays["textures"][ids["env"]]
    p = Pair(fs, cam, setup=lambda r: r.set_sampling_options(ibl_importance=importance))
    try:
        was = film(p.a)

        def repaint():
            # (synthetic_envmap ignores its seed: the other content is the second map's)
            tex[...] = other * np.float32(1.5)
            tex[..., 3] = 1.0
        p.step(repaint, lambda r: r.UpdateTexture(fs, ids["env"]), what="environment map")
        assert film(p.a) != was
    finally:
        p.close()


def test_texture_of_another_size_is_refused():
    fs, cam = scenedefs.toon_room()
    r = new_context(fs, cam)
    try:
        before = film(r)
        big = np.ones((2, 64, 4), np.float32)
        td = L.TextureDesc(big.ctypes.data, 64, 2)
        assert r._l.atn_update_texture(r._ctx, 0, C.byref(td)) == UNSUPPORTED
        assert r._l.atn_last_error(r._ctx).decode() == "a texture update keeps the texture's size"
        assert film(r) == before
    finally:
        r.close()


# ---- 7. the rendering config --------------------------------------------------------------------------------------------------------
def test_config_edits():
    fs, cam, ids, other = _env_sponza()
    cfg = fs.desc.config
    edit = lambda r: r.UpdateSceneRenderingConfig(fs)
    p = Pair(fs, cam)
    try:
        steps = [
            ("multiplyer", lambda: setattr(cfg.bg, "multiplyer", 2.5)),
            ("enable_env_map off", lambda: setattr(cfg.bg, "enable_env_map", 0)),
            ("bg_color", lambda: cfg.bg.bg_color.__setitem__(slice(0, 3), [0.9, 0.2, 0.4])),
            ("enable_env_map on", lambda: setattr(cfg.bg, "enable_env_map", 1)),
            ("envmap_tex_idx", lambda: setattr(cfg.bg, "envmap_tex_idx", ids["other"])),
            ("bvh_hit_min", lambda: setattr(cfg, "bvh_hit_min", 0.05)),
        ]
        for what, change in steps:
            p.step(change, edit, what=what)

        def everything():
            cfg.bg.multiplyer, cfg.bg.envmap_tex_idx, cfg.bvh_hit_min = 0.75, ids["env"], 1e-3
            cfg.bg.bg_color[:] = [0.1, 0.1, 0.3]
        p.step(everything, edit, what="all at once")
    finally:
        p.close()
    # with the table sampler: another map and another multiplyer mean other tables
    p = Pair(fs, cam, setup=lambda r: r.set_sampling_options(ibl_importance=True))
    try:
        def other_map():
            cfg.bg.envmap_tex_idx, cfg.bg.multiplyer = ids["other"], 1.5
        p.step(other_map, edit, what="envmap_tex_idx under ibl_importance")
    finally:
        p.close()


def test_config_alpha_blending_feature_lines_and_medium_bias():
    # enable_alpha_blending: the alpha room, from off to on
    fs, cam = scenedefs.cornell_box_variant(lights="point")
    mats, names = fs.arrays["materials"], fs.names["materials"]
    mats["baseColor"][names.index("shortBox")][3] = 0.5
    p = Pair(fs, cam)
    try:
        blocked = film(p.a)
        p.step(lambda: setattr(fs.desc.config, "enable_alpha_blending", 1), lambda r: r.UpdateSceneRenderingConfig(fs), what="enable_alpha_blending")
        assert film(p.a) != blocked
    finally:
        p.close()
    # feature_line: other line settings, then off -- npr_render refuses as a fresh upload does
    fs, cam = scenedefs.npr_room()
    p = Pair(fs, cam)
    try:
        p.step(lambda: scenedefs.with_feature_lines((fs, cam), color=(0.8, 0.1, 0.1), width=3.0, albedo_threshold=0.3, normal_threshold=0.25),
               lambda r: r.UpdateSceneRenderingConfig(fs), renderers=("npr_render",), what="feature_line")
        fs.desc.config.feature_line[0] = 0
        p.a.UpdateSceneRenderingConfig(fs)
        with pytest.raises(AtenAmdError, match="feature lines are off"):
            p.a.npr_render(W, H, DEPTH, RR)
    finally:
        p.close()
    # the medium epsilon bias
    fs, cam = scenedefs.cornell_box_smoke()
    p = Pair(fs, cam)
    try:
        p.step(lambda: setattr(fs.desc.config, "epsilon_bias", 0.01), lambda r: r.UpdateSceneRenderingConfig(fs), renderers=("volume_render",), what="medium epsilon bias")
    finally:
        p.close()


# ---- 8. every renderer behind a material edit ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("renderer", ["svgf_render", "restir_render", "ao_render"])
def test_renderers_behind_a_material_edit(renderer):
    fs, cam = scenedefs.cornell_box_variant(lights="mixed")
    mats, names = fs.arrays["materials"], fs.names["materials"]
    wall, box = names.index("backWall"), names.index("tallBox")
    p = Pair(fs, cam)
    try:
        film(p.a, renderer, frames=2)                                   # (a history from before the edit, reset below)

        def change():
            mats["baseColor"][wall] = (0.2, 0.5, 0.9, 1.0)
            mats[box] = material(L.MTRL_GGX, (0.9, 0.8, 0.3), box, roughness=0.25, ior=0.02)
        p.step(change, lambda r: r.updateMaterial(fs), renderers=(renderer,), what=renderer)
    finally:
        p.close()


def test_npr_and_volume_behind_a_material_edit():
    fs, cam = scenedefs.npr_room()
    mats, names = fs.arrays["materials"], fs.names["materials"]
    box = names.index("tallBox")
    p = Pair(fs, cam)
    try:
        def change():
            mats["baseColor"][box] = (0.3, 0.8, 0.5, 1.0)
            mats["baseColor"][names.index("leftWall")] = (0.9, 0.9, 0.1, 1.0)
        p.step(change, lambda r: r.updateMaterial(fs), renderers=("npr_render",), what="npr_render")
    finally:
        p.close()
    fs, cam = scenedefs.cornell_box_smoke()
    mats, names = fs.arrays["materials"], fs.names["materials"]
    smoke = names.index("medium")
    p = Pair(fs, cam)
    try:
        def thicker():
            from aten_amd.scene.builder import write_medium
            write_medium(mats[smoke], 0.3, 0.0, 1.25, (1.0, 0.0, 0.0))
        p.step(thicker, lambda r: r.updateMaterial(fs, first=smoke, n=1), renderers=("volume_render",), what="sigma_s and g")
    finally:
        p.close()


# ---- 9. what a re-upload would lose -------------------------------------------------------------------------------------------------
def test_edit_keeps_skins_and_rebuilt_lists():
    n_bones = 4
    b, oid, cam, sv = scenedefs.skinned_room(24, 12, n_bones)
    fs = b.build()
    o = fs.arrays["objects"][oid]
    t0, n = int(o["triangle_id"]), int(o["triangle_num"])
    v0 = int(fs.arrays["triangles"][t0:t0 + n]["idx"].min())
    lst = fs.blas_index[oid]
    mats, names = fs.arrays["materials"], fs.names["materials"]
    wall = names.index("leftWall")

    def tick(r, skin, k):
        r.skin_update(skin, scenedefs.skinned_pose(0.9 * k + 0.4, n_bones))
        r.skin_compute(skin, k == 0, want_bbox=False)
        r.lbvh_rebuild_list_skinned(lst, skin)

    a = new_context(fs, cam)
    try:
        skin = a.skin_create(sv, v0, t0, n, n_bones)
        tick(a, skin, 0)
        rebuilt = a.bvh_list_bytes(lst).tobytes()
        mats["baseColor"][wall] = (0.1, 0.7, 0.9, 1.0)
        a.updateMaterial(fs, first=wall, n=1)
        assert a.bvh_list_bytes(lst).tobytes() == rebuilt               # the edit never touches the node image
        b_ = new_context(fs, cam)                                       # uploads the edited scene, does the same ticks
        try:
            skin_b = b_.skin_create(sv, v0, t0, n, n_bones)
            tick(b_, skin_b, 0)
            assert film(a) == film(b_)
            tick(a, skin, 1)                                            # the skin handle is alive
            tick(b_, skin_b, 1)
            assert a.bvh_list_bytes(lst).tobytes() == b_.bvh_list_bytes(lst).tobytes()
            assert film(a) == film(b_)
        finally:
            b_.close()
    finally:
        a.close()


# ---- 10. around the edit ------------------------------------------------------------------------------------------------------------
def _edited_twice(fs):
    mats, names = fs.arrays["materials"], fs.names["materials"]
    lights = fs.arrays["lights"]
    wall = names.index("rightWall")

    def change():
        mats["baseColor"][wall] = (0.9, 0.4, 0.1, 1.0)
        lights["intensity"][0] = 90.0
    return change


def test_edit_between_groups_of_frames_in_flight():
    w, h = 100, 52
    fs, cam = scenedefs.cornell_box()
    change = _edited_twice(fs)
    fs2, _ = scenedefs.cornell_box()
    a = new_context(fs, cam, w, h, setup=lambda r: r.set_frames_in_flight(4))
    plain = new_context(fs2, cam, w, h)
    try:
        for r in (a, plain):
            for f in range(4):
                r.render(w, h, DEPTH, RR, frame=f, download=False)
        change()
        a.updateMaterial(fs)
        a.updateLight(fs)
        _edited_twice(fs2)()
        plain.updateMaterial(fs2)
        plain.updateLight(fs2)
        for r in (a, plain):
            for f in range(4, 8):
                r.render(w, h, DEPTH, RR, frame=f, download=False)
        got = a.download_film().tobytes()
        assert got == plain.download_film().tobytes()
        # ... and the plain context is itself what a fresh upload gives: frames 4-7 accumulate on the film of frames 0-3, so compare
        # from a reset
        fresh = new_context(fs, cam, w, h)
        try:
            assert film(a, w=w, h=h) == film(fresh, w=w, h=h)
        finally:
            fresh.close()
    finally:
        a.close()
        plain.close()


def test_regenerated_burst_after_an_edit():
    fs, cam = scenedefs.cornell_box()
    a = new_context(fs, cam, setup=lambda r: r.set_regeneration(True))
    try:
        a.render_burst(W, H, 2, DEPTH, RR, spp=2)
        _edited_twice(fs)()
        a.updateMaterial(fs)
        a.updateLight(fs)
        b = new_context(fs, cam, setup=lambda r: r.set_regeneration(True))
        try:
            a.reset()
            b.reset()
            assert a.render_burst(W, H, 3, DEPTH, RR, spp=2).tobytes() == b.render_burst(W, H, 3, DEPTH, RR, spp=2).tobytes()
        finally:
            b.close()
    finally:
        a.close()


def test_mgpu_edits_on_every_shard():
    w, h = 100, 52
    fs, cam = scenedefs.toon_room()
    ramp = fs.names["textures"].index("ramp4")
    camera = create_camera(cam["pos"], cam["at"], cam["vfov"], w, h)
    m = MultiGpuPathTracing([0, 0])
    try:
        m.UpdateSceneData(fs)
        m.updateCamera(camera)
        m.initSampler(w, h, 0)
        m.render(w, h, DEPTH, RR, frame=0)
        fs.arrays["materials"]["baseColor"][fs.names["materials"].index("leftWall")] = (0.2, 0.9, 0.3, 1.0)
        fs.arrays["lights"]["intensity"][0] = 120.0
        npr_target_lights(fs)["pos"][0] = (-0.4, 1.5, 1.0, 1.0)
        fs.arrays["textures"][ramp][...] = scenedefs.toon_ramp((0.1, 0.5, 0.7, 0.95))
        fs.desc.config.bg.bg_color[:] = [0.2, 0.1, 0.4]
        m.updateMaterial(fs)
        m.updateLight(fs)
        m.updateLight(fs, npr_target=True)
        m.UpdateTexture(fs, ramp)
        m.UpdateSceneRenderingConfig(fs)
        m.reset()
        got = None
        for f in range(FRAMES):
            got = m.render(w, h, DEPTH, RR, frame=f)
        single = new_context(fs, cam, w, h)
        try:
            assert got.tobytes() == film(single, w=w, h=h)
        finally:
            single.close()
    finally:
        m.close()


# ---- 11. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    fs, cam = scenedefs.toon_room()
    mats, lights = fs.arrays["materials"], fs.arrays["lights"]
    n_m, n_l, n_t = len(mats), len(lights), int(fs.desc.n_textures)
    r = PathTracing(0)
    try:
        l = r._l
        said = lambda: l.atn_last_error(r._ctx).decode()
        cfg = C.byref(fs.desc.config)
        tex0 = C.byref(C.cast(fs.desc.textures, C.POINTER(L.TextureDesc))[0])
        # before an upload
        for rc in (l.atn_update_materials(r._ctx, mats.ctypes.data, n_m, 0), l.atn_update_lights(r._ctx, lights.ctypes.data, n_l, 0, 0),
                   l.atn_update_texture(r._ctx, 0, tex0), l.atn_update_rendering_config(r._ctx, cfg)):
            assert rc == NO_SCENE and said() == "atn_upload_scene has not been called"
        r.UpdateSceneData(fs)
        r.updateCamera(create_camera(cam["pos"], cam["at"], cam["vfov"], W, H))
        r.initSampler(W, H, 0)
        before = film(r)
        # null pointers
        assert l.atn_update_materials(r._ctx, None, n_m, 0) == INVALID_ARG and said() == "null material array"
        assert l.atn_update_lights(r._ctx, None, n_l, 0, 0) == INVALID_ARG and said() == "null light array"
        assert l.atn_update_lights(r._ctx, None, 1, 0, 1) == INVALID_ARG
        assert l.atn_update_texture(r._ctx, 0, None) == INVALID_ARG and said() == "null texture"
        assert l.atn_update_rendering_config(r._ctx, None) == INVALID_ARG and said() == "null rendering config"
        assert l.atn_update_materials(None, mats.ctypes.data, n_m, 0) == INVALID_ARG
        # ranges past the end
        assert l.atn_update_materials(r._ctx, mats.ctypes.data, n_m, 1) == INVALID_ARG and said() == "material range outside the uploaded scene"
        assert l.atn_update_materials(r._ctx, mats.ctypes.data, 1, n_m) == INVALID_ARG
        assert l.atn_update_materials(r._ctx, mats.ctypes.data, 0xFFFFFFFF, 2) == INVALID_ARG
        assert l.atn_update_lights(r._ctx, lights.ctypes.data, n_l + 1, 0, 0) == INVALID_ARG and said() == "light range outside the uploaded scene"
        assert l.atn_update_lights(r._ctx, lights.ctypes.data, 2, 0, 1) == INVALID_ARG        # (one NPR target light)
        assert l.atn_update_texture(r._ctx, n_t, tex0) == INVALID_ARG and l.atn_update_texture(r._ctx, -1, tex0) == INVALID_ARG
        # content the upload refuses: the same status and message as atn_upload_scene of the same scene
        bad = mats.copy()
        bad["baseColor"][1] = (0.0, 1.0, 0.0, 1.0)                      # (a valid change in the same call must not get through)
        bad["albedoMap"][2] = n_t
        assert l.atn_update_materials(r._ctx, bad.ctypes.data, n_m, 0) == UNSUPPORTED and said() == "material texture index out of range"
        toon = [i for i in range(n_m) if int(mats["type"][i]) == L.MTRL_TOON][0]
        bad = mats.copy()
        bad["toon"]["target_light_idx"][toon] = 1
        assert l.atn_update_materials(r._ctx, bad[toon:].ctypes.data, 1, toon) == UNSUPPORTED and said() == "toon material's target light index out of range"
        ibl = lights[:1].copy()
        ibl["type"], ibl["attrib"], ibl["arealight_objid"], ibl["envmapidx"] = L.LIGHT_IBL, L.LATTR_INFINITE | L.LATTR_IBL, -1, n_t
        assert l.atn_update_lights(r._ctx, ibl.ctypes.data, 1, 0, 0) == UNSUPPORTED and said() == "IBL light's environment map index out of range"
        far = lights[:1].copy()
        far["arealight_objid"] = int(fs.desc.n_objects)
        assert l.atn_update_lights(r._ctx, far.ctypes.data, 1, 0, 0) == UNSUPPORTED and said() == "light refers to an object id out of range"
        assert l.atn_update_lights(r._ctx, far.ctypes.data, 1, 0, 1) == UNSUPPORTED and said() == "NPR target light refers to an object id out of range"
        bad_cfg = L.SceneRenderingConfig.from_buffer_copy(fs.desc.config)
        bad_cfg.bg.envmap_tex_idx = n_t
        bad_cfg.bg.bg_color[:] = [1.0, 0.0, 0.0]
        assert l.atn_update_rendering_config(r._ctx, C.byref(bad_cfg)) == UNSUPPORTED and said() == "the config's environment map texture index out of range"
        # ... which is what the upload says to the same content
        keep = int(fs.desc.config.bg.envmap_tex_idx)
        fs.desc.config.bg.envmap_tex_idx = n_t
        other = PathTracing(0)
        try:
            assert other._l.atn_upload_scene(other._ctx, C.cast(fs.ref(), C.c_void_p)) == UNSUPPORTED
            assert other._l.atn_last_error(other._ctx).decode() == "the config's environment map texture index out of range"
            fs.desc.config.bg.envmap_tex_idx = keep
            keep_map = int(mats["albedoMap"][2])
            mats["albedoMap"][2] = n_t
            assert other._l.atn_upload_scene(other._ctx, C.cast(fs.ref(), C.c_void_p)) == UNSUPPORTED
            assert other._l.atn_last_error(other._ctx).decode() == "material texture index out of range"
            mats["albedoMap"][2] = keep_map
        finally:
            fs.desc.config.bg.envmap_tex_idx = keep
            other.close()
        # nothing changed: the next film is the film before the attempts, and the context still takes a good edit
        assert film(r) == before
        assert l.atn_update_materials(r._ctx, mats.ctypes.data, n_m, 0) == 0
        assert film(r) == before
    finally:
        r.close()
