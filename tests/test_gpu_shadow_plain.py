"""The plain shadow job (DevScene::shadow_plain, host/scene_upload.hpp: shadow_plain_class; device/kernels.hpp, ShadowJob; docs/TRACE_RAY_COST.md):
where every light is infinite and none is an area light with an object, the ALPHA = false shadow job of render()'s serial loop reads no
light record -- its stop distance is +inf, a blocked ray finishes without touching memory, a ray that reaches its light adds sh_c to
contrib (or, in a deferred-NEE frame, sets nee_reached).  It re-derives nothing but scene constants, so every film is BYTE-equal to the
one a context created under ATEN_AMD_SHADOW_PLAIN=0 (the flag stays off: the generic job) renders, counted frames count the same, and a
light edit decides the flag again.

Frames are 64 x 36 and a ragged 100 x 52 (against the 8 x 8 tiles and the 1024-entry chunks); every case runs on the plain walk and with
ATEN_AMD_TRACE=r, which puts the lane-refilling walk under test at this size.  Each case renders 4 progressive frames."""
import os

import numpy as np
import pytest

from aten_amd import layout as L
from aten_amd.scene import scenedefs
from aten_amd.scene.builder import SceneBuilder
from aten_amd.scene.camera import create_camera

pytestmark = pytest.mark.gpu

SIZES = [(64, 36), (100, 52)]
WALKS = ["plain", "refill"]


def _directional(b):
    l = np.zeros((), L.LIGHT_PARAM)
    l["type"] = L.LIGHT_DIRECTION
    l["attrib"] = L.LATTR_SINGULAR | L.LATTR_INFINITE
    d = np.array([-0.2, -0.6, -1.0], np.float32)
    d /= np.linalg.norm(d)
    l["dir"] = (d[0], d[1], d[2], 0.0)
    l["light_color"] = (1.0, 0.95, 0.9)
    l["innerAngle"] = l["outerAngle"] = np.pi
    l["scale"], l["intensity"] = 1.0, 3.0
    l["arealight_objid"], l["envmapidx"] = -1, -1
    b.lights.append(l)


def _stencil_alpha_room(light):
    """The occluder scene of the deferral tests (tests/test_gpu_nee_deferral.py): the Cornell box's surfaces StencilType::ALWAYS, its two
    boxes STENCIL, an alpha-textured pane under the light, alpha blending on -- the ALPHA = true shadow job with restarts behind ignored
    surfaces.  light = "point" is that scene; "directional" puts it under an infinite light, where the flag is on and the job must not
    read it."""
    b = SceneBuilder()

    def create_mtrl(name, mtype, clr, albedo, nml):
        m = b.add_material(name, L.MTRL_GGX if name == "floor" else L.MTRL_DIFFUSE, clr, **(dict(roughness=0.2, ior=0.01) if name == "floor" else {}))
        b.materials[m][1]["stencil_type"] = 2 if name in ("shortBox", "tallBox") else 1
        return m

    objs = b.load_obj(os.path.join(scenedefs.ASSETS, "cornellbox", "orig.obj"), create_mtrl=create_mtrl, separate_objs=True,
                      normal_on_the_fly=True)
    for o in objs:
        if b.objects[o]["name"] != "light":
            b.create_instance(o)
    tex = np.ones((8, 8, 4), np.float32)
    tex[..., :3] = 0.9
    tex[(np.add.outer(np.arange(8), np.arange(8)) % 2) == 0, 3] = 0.4
    pane = b.add_material("pane", L.MTRL_DIFFUSE, (1.0, 1.0, 1.0, 1.0), albedo_map=b.add_texture("alpha_checker", tex))
    q = np.array([[-0.6, 1.4, -0.4], [0.6, 1.4, -0.4], [0.6, 1.4, 0.6], [-0.6, 1.4, 0.6]], np.float32)
    uv = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float32)
    b.create_instance(b.add_mesh("pane", q, [[0, 1, 2], [0, 2, 3]], pane, uvs=uv))
    b.config.enable_alpha_blending = 1
    if light == "point":
        b.add_point_light((0.1, 1.8, 0.2), (1.0, 0.9, 0.8), 30.0)
    else:
        _directional(b)
    b.set_background((0.1, 0.15, 0.2))
    return b.build(), dict(pos=(0.0, 1.0, 3.0), at=(0.0, 1.0, 0.0), vfov=45.0)


_SCENES = {
    "directional": lambda: scenedefs.cornell_box_variant(lights="directional"),
    "ibl_and_point": lambda: scenedefs.sponza_lod(add_lights=lambda b, lo, hi, cam: b.add_point_light((0.0, 1.5, 0.0), (1.0, 0.9, 0.8), 20.0)),
    "stencil_alpha": lambda: _stencil_alpha_room("point"),
    "stencil_alpha_directional": lambda: _stencil_alpha_room("directional"),
}
_built = {}


def _scene(name, sponza=None, cornell=None):
    if name == "sponza":
        return sponza
    if name == "cornell":
        return cornell
    if name not in _built:
        _built[name] = _SCENES[name]()
    return _built[name]


def _ctx(monkeypatch, walk, plain, scene, w, h, shard=None, in_flight=None, lookahead=None):
    """A context created with the hook off (plain = False: ATEN_AMD_SHADOW_PLAIN=0) or as a caller gets it."""
    from aten_amd.renderer import PathTracing
    if walk == "refill":
        monkeypatch.setenv("ATEN_AMD_TRACE", "r")
    else:
        monkeypatch.delenv("ATEN_AMD_TRACE", raising=False)
    for name in ("ATEN_AMD_NEE_DEFERRAL", "ATEN_AMD_RR_LOOKAHEAD", "ATEN_AMD_FUSE"):
        monkeypatch.delenv(name, raising=False)
    if plain:
        monkeypatch.delenv("ATEN_AMD_SHADOW_PLAIN", raising=False)
    else:
        monkeypatch.setenv("ATEN_AMD_SHADOW_PLAIN", "0")
    fs, cam = scene
    r = PathTracing(0)
    r.UpdateSceneData(fs)
    r.updateCamera(create_camera(cam["pos"], cam["at"], cam["vfov"], w, h))
    r.initSampler(w, h, 0)
    if lookahead is not None:
        r.set_rr_lookahead(lookahead)
    if shard:
        r.setScreenShard(*shard)
    if in_flight:
        r.set_frames_in_flight(in_flight)
    return r


def _films(r, w, h, depth, rr, spp=1, brk=True, frames=4, overlap=False, deferral=0, profile=False):
    r.set_nee_deferral(deferral)
    r.reset()
    if overlap:
        for f in range(frames):
            r.render(w, h, depth, rr, spp=spp, frame=f, break_on_terminate=brk, download=False)
        r.synchronize()
        return [r.download_film().tobytes()]
    return [r.render(w, h, depth, rr, spp=spp, frame=f, break_on_terminate=brk, profile=profile).tobytes() for f in range(frames)]


# (scene, maxDepth, russianRouletteDepth, spp, break_on_terminate, (rank, world) or None, frames in flight, look-ahead mode or None =
#  default, deferral mode)
_CASES = {
    "sponza_depth5_rr3": ("sponza", 5, 3, 1, True, None, 0, None, 0),
    "sponza_depth5_rr3_without_lookahead": ("sponza", 5, 3, 1, True, None, 0, 0, 0),
    "directional_room": ("directional", 5, 3, 1, True, None, 0, None, 0),
    "stencil_always_and_alpha_texture": ("stencil_alpha", 5, 3, 1, True, None, 0, None, 0),
    "stencil_always_and_alpha_texture_directional": ("stencil_alpha_directional", 5, 3, 1, True, None, 0, None, 0),
    "sponza_deferred_nee": ("sponza", 5, 3, 1, True, None, 0, None, 1),
    "directional_room_deferred_nee": ("directional", 5, 3, 1, True, None, 0, None, 1),
    "depth1_first_vertex_is_last": ("sponza", 1, 3, 1, True, None, 0, None, 0),
    "depth8_rr3": ("sponza", 8, 3, 1, True, None, 0, None, 0),
    "spp2_break": ("sponza", 5, 3, 2, True, None, 0, None, 0),
    "spp2_all_samples": ("sponza", 5, 3, 2, False, None, 0, None, 0),
    "spp8_break": ("sponza", 5, 3, 8, True, None, 0, None, 0),
    "spp8_all_samples": ("sponza", 5, 3, 8, False, None, 0, None, 0),
    "shard_1_of_2": ("sponza", 5, 3, 1, True, (1, 2), 0, None, 0),
    "three_frames_in_flight": ("sponza", 5, 3, 1, True, None, 3, None, 0),
}


@pytest.mark.parametrize("walk", WALKS)
@pytest.mark.parametrize("case", sorted(_CASES))
def test_films_are_byte_equal_with_and_without_the_plain_shadow_job(monkeypatch, sponza, cornell, case, walk):
    name, depth, rr, spp, brk, shard, in_flight, lookahead, deferral = _CASES[case]
    scene = _scene(name, sponza, cornell)
    for w, h in SIZES:
        films = []
        for plain in (False, True):
            r = _ctx(monkeypatch, walk, plain, scene, w, h, shard=shard, in_flight=in_flight or None, lookahead=lookahead)
            try:
                if deferral:
                    r.set_nee_deferral(deferral)
                    assert r.nee_deferral_active()      # (else nee_reached is never set from the plain finish)
                films.append(_films(r, w, h, depth, rr, spp, brk, overlap=bool(in_flight), deferral=deferral))
                if deferral:
                    st = r.nee_deferral_stats()
                    assert 0 < st["reached"] <= st["cast"], st      # (some ray reached its light: the evaluation launch had work)
            finally:
                r.close()
        assert films[1] == films[0], "%s %dx%d: films differ" % (case, w, h)
        assert any(np.frombuffer(f, np.float32).reshape(-1, 4)[:, :3].any() for f in films[0]), "%s: a black film compares nothing" % case


@pytest.mark.parametrize("walk", WALKS)
@pytest.mark.parametrize("name", ["ibl_and_point", "cornell"])
def test_scenes_with_a_finite_light_or_a_lamp_object_launch_identically(monkeypatch, sponza, cornell, name, walk):
    """IBL + a point light, and the Cornell box under its area lamp: the flag is off in both contexts -- the same launches (counts per
    kernel of profiled frames), the same films."""
    scene = _scene(name, sponza, cornell)
    for w, h in SIZES:
        got = []
        for plain in (False, True):
            r = _ctx(monkeypatch, walk, plain, scene, w, h)
            try:
                r.reset_kernel_times()
                films = _films(r, w, h, 5, 3, profile=True)
                got.append((films, {k: n for k, (ms, n) in r.kernel_times().items()}))
            finally:
                r.close()
        assert got[1][1] == got[0][1], "%s %dx%d: launch counts differ" % (name, w, h)
        assert sum(got[0][1].values()) > 0
        assert got[1][0] == got[0][0], "%s %dx%d: films differ" % (name, w, h)


@pytest.mark.parametrize("walk", WALKS)
def test_regenerated_burst_and_svgf_frame_are_unchanged(monkeypatch, sponza, walk):
    """The regenerated pool (REGEN shadow job) and SVGF's path pass keep what they launched: the same bytes with the hook on and off."""
    w, h = SIZES[1]
    got = []
    for plain in (False, True):
        r = _ctx(monkeypatch, walk, plain, sponza, w, h)
        try:
            r.set_regeneration(True)
            r.reset()
            burst = r.render_burst(w, h, 3, 5, 3, spp=4, frame=0).tobytes()
            r.set_regeneration(False)
            r.reset()
            r.svgf_reset()
            svgf = [r.svgf_render(w, h, 5, 3, frame=f, compute_motion=True).tobytes() for f in range(2)]
            got.append((burst, svgf))
        finally:
            r.close()
    assert got[1][0] == got[0][0], "regenerated burst"
    assert got[1][1] == got[0][1], "SVGF frames"


@pytest.mark.parametrize("walk", WALKS)
@pytest.mark.parametrize("name", ["sponza", "directional", "cornell"])
def test_counted_frames_count_the_same(monkeypatch, sponza, cornell, name, walk):
    """A counted frame (the unfused, counting kernels: generic by construction) gives the same film and the same atn_get_stats."""
    scene = _scene(name, sponza, cornell)
    w, h = SIZES[1]
    got = []
    for plain in (False, True):
        r = _ctx(monkeypatch, walk, plain, scene, w, h)
        try:
            r.reset()
            film = r.render(w, h, 5, 3, frame=0, count_stats=True).tobytes()
            got.append((film, r.stats()))
        finally:
            r.close()
    assert got[1][1] == got[0][1]
    assert got[0][1]["shadow_rays"] > 0
    assert got[1][0] == got[0][0]


@pytest.mark.parametrize("walk", WALKS)
def test_a_light_edit_decides_the_flag_again(monkeypatch, walk):
    """A room under one directional light (flag on) whose light becomes a point light (flag off) and a directional light again
    (updateLight): the films of each stage equal those of a context uploaded in that state, with the hook on and with it off."""
    fs, cam = scenedefs.cornell_box_variant(lights="directional")
    lights = fs.arrays["lights"]
    was = lights[0].copy()
    w, h = SIZES[1]

    def to_point():
        lights["type"][0] = L.LIGHT_POINT
        lights["attrib"][0] = L.LATTR_SINGULAR
        lights["pos"][0] = (0.3, 1.6, 0.4, 1.0)

    def to_directional():
        lights[0] = was

    def fresh():        # contexts uploaded in the scene's present state: hook off, hook on
        out = []
        for plain in (False, True):
            r = _ctx(monkeypatch, walk, plain, (fs, cam), w, h)
            try:
                out.append(_films(r, w, h, 5, 3))
            finally:
                r.close()
        assert out[1] == out[0]
        return out[0]

    edited = _ctx(monkeypatch, walk, True, (fs, cam), w, h)
    try:
        directional = _films(edited, w, h, 5, 3)
        assert directional == fresh()
        to_point()
        edited.updateLight(fs)
        point = _films(edited, w, h, 5, 3)
        assert point == fresh(), "directional -> point"
        assert point != directional
        to_directional()
        edited.updateLight(fs)
        assert _films(edited, w, h, 5, 3) == directional, "point -> directional"
    finally:
        edited.close()
