"""The deferred NEE (atn_set_nee_deferral, include/aten_amd.h; device/kernels.hpp, PathBuffers::nee_reached; docs/NEE_DEFERRAL.md): in a
deferred frame shade casts a vertex's shadow ray from the light sample's geometry alone, and the rest of the sample is evaluated after the
ray has been traced, for the rays that reached their light, by a launch that replays those vertices.  Nothing of that may reach the
film: every film in mode 1 (forced on) is BYTE-equal to the one rendered in mode 0.  The policy (mode 2) defers only where
every light is infinite; a new context starts in mode 0; CarPaint and toon scenes, counted frames and the passes that are not render()'s serial loop stay eager; and
the stats have to show that the evaluation launch sees the rays it should.

Frames are 64 x 36 and a ragged 100 x 52; every case runs on the plain walk and with ATEN_AMD_TRACE=r (read when the context is
created), which puts the lane-refilling walk under test at this size.  Each case renders 4 progressive frames."""
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


def _stencil_alpha_room():
    """The Cornell box's geometry under a point light: the room's surfaces are StencilType::ALWAYS, the two boxes STENCIL (shadow
    rays of the room's vertices carry kShadowStencilFlag and restart behind the boxes), and a pane with an alpha-textured albedo
    (a checkerboard of alpha 0.4 / 1.0) hangs under the light with alpha blending on: restarts behind ignored surfaces."""
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
    b.add_point_light((0.1, 1.8, 0.2), (1.0, 0.9, 0.8), 30.0)
    b.set_background((0.1, 0.15, 0.2))
    return b.build(), dict(pos=(0.0, 1.0, 3.0), at=(0.0, 1.0, 0.0), vfov=45.0)


_SCENES = {
    # IBL (2 draws) + a point light (none): the light pick is a draw
    "ibl_and_point": lambda: scenedefs.sponza_lod(add_lights=lambda b, lo, hi, cam: b.add_point_light((0.0, 1.5, 0.0), (1.0, 0.9, 0.8), 20.0)),
    "sphere": lambda: scenedefs.cornell_box_variant(lights="sphere"),          # (the variants carry a Disney box: material set Disney)
    "point": lambda: scenedefs.cornell_box_variant(lights="point"),
    "spot": lambda: scenedefs.cornell_box_variant(lights="spot"),
    "directional": lambda: scenedefs.cornell_box_variant(lights="directional"),
    "mixed": lambda: scenedefs.cornell_box_variant(lights="mixed"),
    "analytic": lambda: scenedefs.cornell_box_variant(lights="area", extra_materials="rough"),
    "stencil_alpha": _stencil_alpha_room,
    "carpaint": lambda: scenedefs.cornell_box_variant(lights="directional", extra_materials="carpaint"),
    "toon": lambda: scenedefs.toon_room(target="point"),
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


def _ctx(monkeypatch, walk, scene, w, h, shard=None, in_flight=None, lookahead=None, ibl_importance=False):
    from aten_amd.renderer import PathTracing
    if walk == "refill":
        monkeypatch.setenv("ATEN_AMD_TRACE", "r")
    else:
        monkeypatch.delenv("ATEN_AMD_TRACE", raising=False)
    monkeypatch.delenv("ATEN_AMD_NEE_DEFERRAL", raising=False)
    monkeypatch.delenv("ATEN_AMD_RR_LOOKAHEAD", raising=False)
    fs, cam = scene
    r = PathTracing(0)
    r.UpdateSceneData(fs)
    r.updateCamera(create_camera(cam["pos"], cam["at"], cam["vfov"], w, h))
    r.initSampler(w, h, 0)
    if ibl_importance:
        r.set_sampling_options(ibl_importance=True)
    if lookahead is not None:
        r.set_rr_lookahead(lookahead)
    if shard:
        r.setScreenShard(*shard)
    if in_flight:
        r.set_frames_in_flight(in_flight)
    return r


def _films(r, mode, w, h, depth, rr, spp=1, brk=True, frames=4, overlap=False):
    """`frames` progressive frames in deferral mode `mode` (a list: one mode per frame), each film as bytes (overlap: frames enqueued
    back to back, the last film only)."""
    modes = mode if isinstance(mode, (list, tuple)) else [mode] * frames
    r.set_nee_deferral(modes[0])
    r.reset()
    if overlap:
        for f in range(frames):
            r.render(w, h, depth, rr, spp=spp, frame=f, break_on_terminate=brk, download=False)
        r.synchronize()
        return [r.download_film().tobytes()]
    out = []
    for f in range(frames):
        r.set_nee_deferral(modes[f])
        out.append(r.render(w, h, depth, rr, spp=spp, frame=f, break_on_terminate=brk).tobytes())
    return out


# (scene, maxDepth, russianRouletteDepth, spp, break_on_terminate, (rank, world) or None, frames in flight, look-ahead mode or None =
#  default, IBL importance sampler)
_CASES = {
    "sponza_depth5_rr3": ("sponza", 5, 3, 1, True, None, 0, None, False),
    "sponza_depth5_rr3_without_lookahead": ("sponza", 5, 3, 1, True, None, 0, 0, False),
    "sponza_ibl_and_point_light_pick": ("ibl_and_point", 5, 3, 1, True, None, 0, None, False),
    "sponza_ibl_importance_table": ("sponza", 5, 3, 1, True, None, 0, None, True),
    "forced_area_light_polygons": ("cornell", 5, 3, 1, True, None, 0, None, False),
    "forced_sphere_light": ("sphere", 5, 3, 1, True, None, 0, None, False),
    "forced_point_light_disney": ("point", 5, 3, 1, True, None, 0, None, False),
    "forced_spot_light": ("spot", 5, 3, 1, True, None, 0, None, False),
    "forced_directional_light": ("directional", 5, 3, 1, True, None, 0, None, False),
    "forced_four_kinds_light_pick": ("mixed", 5, 1, 1, True, None, 0, None, False),
    "forced_analytic_set": ("analytic", 5, 3, 1, True, None, 0, None, False),
    "stencil_always_and_alpha_texture": ("stencil_alpha", 5, 3, 1, True, None, 0, None, False),
    "depth1_first_vertex_is_last": ("sponza", 1, 3, 1, True, None, 0, None, False),
    "depth8_rr3": ("sponza", 8, 3, 1, True, None, 0, None, False),
    "spp2_break": ("sponza", 5, 3, 2, True, None, 0, None, False),
    "spp2_all_samples": ("sponza", 5, 3, 2, False, None, 0, None, False),
    "spp8_break": ("sponza", 5, 3, 8, True, None, 0, None, False),
    "spp8_all_samples": ("sponza", 5, 3, 8, False, None, 0, None, False),
    "shard_1_of_3": ("sponza", 5, 3, 1, True, (1, 3), 0, None, False),
    "three_frames_in_flight": ("sponza", 5, 3, 1, True, None, 3, None, False),
}


@pytest.mark.parametrize("walk", WALKS)
@pytest.mark.parametrize("case", sorted(_CASES))
def test_films_are_byte_equal_with_and_without_deferral(monkeypatch, sponza, cornell, case, walk):
    name, depth, rr, spp, brk, shard, in_flight, lookahead, importance = _CASES[case]
    scene = _scene(name, sponza, cornell)
    for w, h in SIZES:
        r = _ctx(monkeypatch, walk, scene, w, h, shard=shard, in_flight=in_flight or None, lookahead=lookahead, ibl_importance=importance)
        try:
            r.set_nee_deferral(1)
            assert r.nee_deferral_active()          # (else the comparison below compares a thing with itself)
            want = _films(r, 0, w, h, depth, rr, spp, brk, overlap=bool(in_flight))
            got = _films(r, 1, w, h, depth, rr, spp, brk, overlap=bool(in_flight))
            assert got == want, "%s %dx%d: films differ" % (case, w, h)
            st = r.nee_deferral_stats()
            assert 0 < st["cast"] and st["reached"] <= st["cast"], st      # (the deferred frames did run the evaluation launch)
        finally:
            r.close()


@pytest.mark.parametrize("walk", WALKS)
def test_switching_the_mode_between_frames_of_a_sequence(monkeypatch, sponza, walk):
    w, h = SIZES[1]
    r = _ctx(monkeypatch, walk, sponza, w, h)
    try:
        want = _films(r, 0, w, h, 5, 3)
        assert _films(r, [1, 0, 2, 0], w, h, 5, 3) == want
        assert _films(r, [0, 2, 0, 1], w, h, 5, 3) == want
    finally:
        r.close()


@pytest.mark.parametrize("walk", WALKS)
def test_the_policy_follows_the_lights(monkeypatch, sponza, cornell, walk):
    """Mode 2 (the policy) defers where every light is infinite -- sponza_lod under its environment, a room under a directional
    light -- and stays eager under an area, point or spot light, which mode 1 still defers; mode 0, in which a context starts, is off
    everywhere.  It follows the scene: uploading another one decides again."""
    w, h = SIZES[1]
    r = _ctx(monkeypatch, walk, sponza, w, h)
    try:
        assert not r.nee_deferral_active()          # a new context: mode 0
        r.set_nee_deferral(2)
        assert r.nee_deferral_active()              # the headline scene
        for name, by_default in (("cornell", False), ("point", False), ("spot", False), ("mixed", False), ("directional", True),
                                 ("ibl_and_point", False)):
            r.UpdateSceneData(_scene(name, sponza, cornell)[0])
            assert r.nee_deferral_active() == by_default, name
            r.set_nee_deferral(1)
            assert r.nee_deferral_active(), name
            r.set_nee_deferral(2)
        r.UpdateSceneData(sponza[0])
        assert r.nee_deferral_active()
    finally:
        r.close()


@pytest.mark.parametrize("walk", WALKS)
@pytest.mark.parametrize("name", ["carpaint", "toon"])
def test_carpaint_and_toon_scenes_stay_eager(monkeypatch, name, walk):
    """CarPaint draws in applyNormal and a toon surface ends the path at the hit: the scene does not qualify, says so in every mode,
    and its frames are the frames of mode 0."""
    scene = _scene(name)
    w, h = SIZES[1]
    r = _ctx(monkeypatch, walk, scene, w, h)
    try:
        want = _films(r, 0, w, h, 5, 1)
        for mode in (1, 2):
            r.set_nee_deferral(mode)
            assert not r.nee_deferral_active()
            assert _films(r, mode, w, h, 5, 1) == want
        assert r.nee_deferral_stats() == dict(cast=0, reached=0)
    finally:
        r.close()


@pytest.mark.parametrize("walk", WALKS)
def test_other_passes_ignore_the_mode(monkeypatch, sponza, walk):
    """SVGF's path pass, the regenerated pool and the relaxed-math shade kernel have no deferred flavour: forced on or off, they
    launch what they launched before and produce the same bytes; no deferred frame is counted."""
    w, h = SIZES[1]
    r = _ctx(monkeypatch, walk, sponza, w, h)
    try:
        def svgf(mode):
            r.set_nee_deferral(mode)
            r.svgf_reset()
            return [r.svgf_render(w, h, 5, 3, frame=f, compute_motion=True).tobytes() for f in range(3)]

        def regen(mode):
            r.set_nee_deferral(mode)
            r.set_regeneration(True)
            r.reset()
            out = [r.render(w, h, 5, 3, spp=4, frame=f).tobytes() for f in range(3)]
            r.set_regeneration(False)
            return out

        def relaxed(mode):
            r.set_nee_deferral(mode)
            r.set_shade_math(True)
            active = r.nee_deferral_active()
            r.reset()
            out = [r.render(w, h, 5, 3, frame=f).tobytes() for f in range(3)]
            r.set_shade_math(False)
            return active, out

        r.reset()
        assert svgf(1) == svgf(0)
        r.reset()                       # (zeroes the stats: nothing above or below may count a deferred frame)
        assert regen(1) == regen(0)
        a1, f1 = relaxed(1)
        a0, f0 = relaxed(0)
        assert not a1 and not a0 and f1 == f0
        assert r.nee_deferral_stats() == dict(cast=0, reached=0)
    finally:
        r.close()


@pytest.mark.parametrize("walk", WALKS)
def test_counted_frames_stay_eager(monkeypatch, sponza, walk):
    """A counted frame keeps the reference's accounting: in mode 1 its film and every counter are mode 0's."""
    w, h = SIZES[1]
    r = _ctx(monkeypatch, walk, sponza, w, h)
    try:
        def counted(mode):
            r.set_nee_deferral(mode)
            r.reset()
            film = r.render(w, h, 5, 3, frame=0, count_stats=True).tobytes()
            return film, r.stats(), r.nee_deferral_stats()
        film0, s0, d0 = counted(0)
        film1, s1, d1 = counted(1)
        assert film1 == film0 and s1 == s0
        assert d0 == d1 == dict(cast=0, reached=0)
    finally:
        r.close()


@pytest.mark.parametrize("walk", WALKS)
def test_the_stats_count_the_rays_the_evaluation_sees(monkeypatch, sponza, cornell, walk):
    """After deferred frames reached <= cast, and cast is at least the counted (eager) frame's shadow rays: the deferred shade casts a
    ray for every sample whose geometry is valid, the eager one only where the BSDF pdf is positive as well.  Inside sponza_lod few rays
    reach the environment (the CPU renderer's counters: 2.3 % at 480 x 270) -- the cap of 10 % only proves that the counter counts
    the right thing -- and in the Cornell box, forced, most reach the lamp (CPU: 87 %)."""
    w, h = SIZES[1]
    shares = {}
    for name, scene in (("sponza", sponza), ("cornell", cornell)):
        r = _ctx(monkeypatch, walk, scene, w, h)
        try:
            r.set_nee_deferral(1)
            r.reset()
            r.render(w, h, 5, 3, frame=0, count_stats=True)
            eager_shadow_rays = r.stats()["shadow_rays"]
            r.reset()
            r.render(w, h, 5, 3, frame=0)
            st = r.nee_deferral_stats()
            print(name, "cast", st["cast"], "reached", st["reached"], "eager shadow rays", eager_shadow_rays)
            assert st["reached"] <= st["cast"]
            assert st["cast"] >= eager_shadow_rays > 0
            r.render(w, h, 5, 3, frame=1)
            st2 = r.nee_deferral_stats()
            assert st2["cast"] > st["cast"] and st2["reached"] >= st["reached"]       # it accumulates until reset()
            r.reset()
            assert r.nee_deferral_stats() == dict(cast=0, reached=0)
            shares[name] = st["reached"] / st["cast"]
        finally:
            r.close()
    assert shares["sponza"] < 0.10, shares
    assert shares["cornell"] > 0.5, shares
