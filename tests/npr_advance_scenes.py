"""Scenes of the NPR look-through tests (docs/NPR_ADVANCE.md): two small analytic rooms -- a wall that leaves the right part of the view
to the background, a GGX floor, a point light -- with feature lines on every material.  TEST INFRASTRUCTURE ONLY.

The camera stands at (0, 1, 3) and looks down -z; what a pixel looks through is in the plane z = 0 .. 0.5, the wall at z = -1.
Every region is about 0.6 x 0.6 (more than 100 pixels at 64 x 48) and has a material of its own: the tests find a region by the
material id of the surface the primary ray meets."""
import numpy as np

from aten_amd import layout as L
from aten_amd.scene import scenedefs
from aten_amd.scene.builder import SceneBuilder

CAM = dict(pos=(0.0, 1.0, 3.0), at=(0.0, 1.0, 0.0), vfov=45.0)
QUAD = [[0, 1, 2], [0, 2, 3]]


def _quad_xy(x0, x1, y0, y1, z, back=False):
    """A quad in the plane z, facing +z (the camera), or -z with back=True."""
    p = np.array([[x0, y0, z], [x1, y0, z], [x1, y1, z], [x0, y1, z]], np.float32)
    return p[::-1].copy() if back else p


UV = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float32)


def _room(b, wall_x1):
    wall = b.add_material("wall", L.MTRL_DIFFUSE, (0.7, 0.6, 0.5))
    floor = b.add_material("floor", L.MTRL_GGX, (0.6, 0.6, 0.7), roughness=0.15, ior=1.5)
    b.create_instance(b.add_mesh("wall", _quad_xy(-2.2, wall_x1, 0.0, 2.7, -1.0), QUAD, wall))
    f = np.array([[-2.2, 0.0, 2.6], [2.2, 0.0, 2.6], [2.2, 0.0, -1.0], [-2.2, 0.0, -1.0]], np.float32)
    b.create_instance(b.add_mesh("floor", f, QUAD, floor))
    b.add_point_light((0.2, 2.3, 2.2), (1.0, 1.0, 1.0), 12.0)
    b.set_background((0.25, 0.4, 0.6))
    return wall, floor


def alpha_texture():
    """8 x 8 texels, rgb a soft gradient, alpha 0 / 0.5 / 1 in 2 x 2 blocks."""
    t = np.ones((8, 8, 4), np.float32)
    for y in range(8):
        for x in range(8):
            t[y, x, :3] = (0.3 + 0.1 * (x % 4), 0.8 - 0.05 * y, 0.5)
            t[y, x, 3] = (0.0, 0.5, 1.0)[((x // 2) + (y // 2)) % 3]
    return t


def alpha_room(blending=True):
    """A pane of baseColor.a = 0.5 in front of the wall; a pane whose alpha comes from a texture's texels (0 / 0.5 / 1); a pane in front
    of the background only; stacks of 9 and of 11 panes in front of the wall; a pane above the view, reached only after a bounce off the
    GGX floor.  -> (scene, camera), names: material name -> id."""
    b = SceneBuilder()
    _room(b, 0.9)
    b.config.enable_alpha_blending = 1 if blending else 0
    pane = b.add_material("pane", L.MTRL_DIFFUSE, (0.9, 0.3, 0.2, 0.5))
    tex = b.add_texture("alpha012", alpha_texture())
    tpane = b.add_material("texpane", L.MTRL_DIFFUSE, (1.0, 1.0, 1.0, 1.0), albedo_map=tex)
    sky = b.add_material("skypane", L.MTRL_DIFFUSE, (0.2, 0.8, 0.3, 0.25))
    s9 = b.add_material("stack9", L.MTRL_DIFFUSE, (0.3, 0.4, 0.9, 0.25))
    s11 = b.add_material("stack11", L.MTRL_DIFFUSE, (0.8, 0.8, 0.2, 0.125))
    top = b.add_material("toppane", L.MTRL_DIFFUSE, (0.9, 0.9, 0.9, 0.5))
    b.create_instance(b.add_mesh("pane", _quad_xy(-1.5, -0.9, 1.4, 2.0, 0.0), QUAD, pane))
    b.create_instance(b.add_mesh("texpane", _quad_xy(-0.7, -0.1, 1.4, 2.0, 0.0), QUAD, tpane, uvs=UV))
    b.create_instance(b.add_mesh("skypane", _quad_xy(1.1, 1.6, 1.2, 2.0, 0.0), QUAD, sky))
    for k in range(9):
        b.create_instance(b.add_mesh("stack9_%d" % k, _quad_xy(-1.5, -0.9, 0.5, 1.1, -0.05 * k), QUAD, s9))
    for k in range(11):
        b.create_instance(b.add_mesh("stack11_%d" % k, _quad_xy(-0.7, -0.1, 0.5, 1.1, -0.05 * k), QUAD, s11))
    t = np.array([[-1.0, 2.6, 2.4], [1.0, 2.6, 2.4], [1.0, 2.6, 0.6], [-1.0, 2.6, 0.6]], np.float32)      # faces down
    b.create_instance(b.add_mesh("toppane", t, QUAD, top))
    names = {n: i for i, (n, _) in enumerate(b.materials)}
    return scenedefs.with_feature_lines((b.build(), dict(CAM))), names


def stencil_room(blending=False):
    """STENCIL in front of a front-facing ALWAYS in front of the wall (NONE); STENCIL in front of a back-facing ALWAYS; STENCIL in front
    of the wall; STENCIL in front of nothing; two STENCIL layers in front of an ALWAYS.  Each STENCIL quad has a material of its own
    (the tests find the regions by it).  -> (scene, camera), names."""
    b = SceneBuilder()
    _room(b, 1.1)
    b.config.enable_alpha_blending = 1 if blending else 0

    def mat(name, clr, stencil):
        m = b.add_material(name, L.MTRL_DIFFUSE, clr)
        b.materials[m][1]["stencil_type"] = stencil
        return m

    brow = mat("brow", (0.15, 0.1, 0.05), 1)
    hair = [mat("hair_%s" % n, (0.9, 0.75 - 0.1 * i, 0.2 + 0.1 * i), 2) for i, n in enumerate(("front", "back", "none", "nothing", "two"))]
    b.create_instance(b.add_mesh("hair_front", _quad_xy(-1.5, -0.9, 1.4, 2.0, 0.5), QUAD, hair[0]))
    b.create_instance(b.add_mesh("brow_front", _quad_xy(-1.9, -1.0, 1.3, 2.1, 0.0), QUAD, brow))
    b.create_instance(b.add_mesh("hair_back", _quad_xy(-0.7, -0.1, 1.4, 2.0, 0.5), QUAD, hair[1]))
    b.create_instance(b.add_mesh("brow_back", _quad_xy(-0.75, -0.05, 1.3, 2.1, 0.0, back=True), QUAD, brow))
    b.create_instance(b.add_mesh("hair_none", _quad_xy(0.0, 0.5, 1.4, 2.0, 0.5), QUAD, hair[2]))
    b.create_instance(b.add_mesh("hair_nothing", _quad_xy(1.0, 1.5, 1.2, 2.0, 0.5), QUAD, hair[3]))
    b.create_instance(b.add_mesh("hair_two_a", _quad_xy(-1.5, -0.9, 0.5, 1.1, 0.5), QUAD, hair[4]))
    b.create_instance(b.add_mesh("hair_two_b", _quad_xy(-1.5, -0.9, 0.5, 1.1, 0.3), QUAD, hair[4]))
    b.create_instance(b.add_mesh("brow_two", _quad_xy(-1.9, -1.0, 0.4, 1.2, 0.0), QUAD, brow))
    names = {n: i for i, (n, _) in enumerate(b.materials)}
    return scenedefs.with_feature_lines((b.build(), dict(CAM))), names


ROOMS = {"alpha": alpha_room, "stencil": stencil_room}

# The categories every frame of the tests must hold, by the twin's advance stage: name -> (room, predicate over the stage dict).
# kind x {hit, miss, budget spent} and each CheckStencil verdict; at least FLOOR pixels each at 64 x 48.
FLOOR = 50
CATEGORIES = {
    "alpha/untouched": ("alpha", lambda s: (s["kind"] == 0) & (s["answer"] >= 0)),
    "alpha/hit": ("alpha", lambda s: (s["kind"] == 2) & (s["alpha_end"] == 1)),
    "alpha/miss": ("alpha", lambda s: (s["kind"] == 2) & (s["alpha_end"] == 2) & (s["answer"] < 0)),
    "alpha/budget": ("alpha", lambda s: (s["kind"] == 2) & (s["alpha_end"] == 3) & (s["walks"] == 10)),
    "stencil/untouched": ("stencil", lambda s: (s["kind"] == 0) & (s["verdict"] == 0) & (s["answer"] >= 0)),
    "stencil/true": ("stencil", lambda s: (s["kind"] == 1) & (s["verdict"] == 1) & (s["walks"] == 1)),
    "stencil/true_two_layers": ("stencil", lambda s: (s["kind"] == 1) & (s["verdict"] == 1) & (s["walks"] == 2)),
    "stencil/back_facing": ("stencil", lambda s: (s["kind"] == 0) & (s["verdict"] == 2)),
    "stencil/none": ("stencil", lambda s: (s["kind"] == 0) & (s["verdict"] == 3)),
    "stencil/miss": ("stencil", lambda s: (s["kind"] == 0) & (s["verdict"] == 4)),
}


def category_counts(room, stage):
    return {k: int(np.count_nonzero(f(stage))) for k, (r, f) in CATEGORIES.items() if r == room}
