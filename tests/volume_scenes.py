"""Scenes and pixel sets for the nested-media gate of the volume renderer (tests/test_volume_nested_cpu.py,
tests/test_gpu_volume_nested.py).

Every builder is deterministic.  `nested_shells` puts n concentric Volume boxes around a point light, over a diffuse floor that cuts
through all of them: a camera ray enters shell after shell before it meets the floor, so at iteration k of radiance's loop a path can
hold k media on its stack, and a connection from the floor walks through up to n boundaries.  `slab_row` lines m separate slabs up
between a wall and a light: a connection crosses 2 m boundaries with never more than one medium on its stack.

The handle (`first_decision_masks`).  A pass through a pure medium boundary is bit-exact on the twin and on the device: the hit comes
from the shared walk, the next origin is ray_offset of it, the direction is normalize of the old one.  So a pixel that at iterations
0 .. k-1 has only PASSED boundaries enters iteration k with bit-equal ray, stack and sampler dimension on both sides, and what it
decides at k -- with up to k media on its stack -- can be compared without any allowance but the 2 ulp of logf in the free flight.
The masks come from the twin's captures alone.  A pixel of a mask whose sampled distance lies within NEAR_TIE_ULPS of the hit distance
could legitimately decide the other way; the CPU tests assert that there is NO such pixel in any case the GPU tests use, so nothing is
left out there."""
import numpy as np

from aten_amd import layout as L

F32 = np.float32
NEAR_TIE_ULPS = 4
ITERATIONS = 8                      # MedisumStackSize: the cap of radiance's loop and the depth of the medium stack
WALK_MAX = 64                       # kVolWalkMax: boundaries a connection may cross
BACKGROUND = (0.25, 0.5, 1.0)
SIZES = ((64, 48), (37, 21))        # one size of whole waves, one ragged
FRAMES = (0, 1)
# under this frame setting every connection of the scenes below starts at the first surface a path meets, behind passes only
# (tests/test_volume_nested_cpu.py confirms it on the twin): the connection counters are then exact, not only close
COUNTER_MAX_DEPTH = 1


def shell_half_size(k, n):
    return 2.0 - 1.7 * k / n


def thin(k):
    """Free flights of ~1e7 units: no event, every boundary is a pass."""
    return dict(g=0.0, sigma_a=0.0, sigma_s=1e-7)


def outer_dense(k):
    """The first medium entered is the dense one: events at every stack depth."""
    if k == 0:
        return dict(g=0.4, sigma_a=0.05, sigma_s=0.6)
    return dict(g=-0.4, sigma_a=0.0, sigma_s=1e-3 * (k + 1))


def outer_thin(k):
    """The first medium entered is thin, every later one dense: the current medium is the FIRST on the stack (aten::stack::top() is
    queue_.front()), so almost nothing happens; a renderer that took the newest medium would scatter hundreds of paths."""
    if k == 0:
        return dict(g=0.0, sigma_a=0.0, sigma_s=1e-3)
    return dict(g=0.4, sigma_a=0.5, sigma_s=5.0)


MEDIA = dict(thin=thin, outer_dense=outer_dense, outer_thin=outer_thin)


def _floor(b, y, half):
    m = b.add_material("floor", L.MTRL_DIFFUSE, (0.7, 0.7, 0.7))
    p = np.array([[-half, y, -half], [half, y, -half], [half, y, half], [-half, y, half]], F32)
    b.create_instance(b.add_mesh("floor", p, [[0, 2, 1], [0, 3, 2]], m))        # the normal is +y
    return m


def nested_shells(n, media, floor_half=4.0):
    """n concentric Volume boxes of half-size 2.0 - 1.7 k / n (k = 0 the outermost), a diffuse floor at y = -0.1 through all of
    them, a point light at (0, 0.05, 0) inside the innermost, a constant background.  media(k) -> dict g, sigma_a, sigma_s[, le].
    -> (scene, camera dict, the shells' material ids from the outermost in)."""
    from aten_amd.scene.builder import SceneBuilder
    from aten_amd.scene.scenedefs import _box_mesh
    if isinstance(media, str):
        media = MEDIA[media]
    b = SceneBuilder()
    ids = []
    for k in range(n):
        md = media(k)
        mid = b.add_medium_material("shell%d" % k, md["g"], md["sigma_a"], md["sigma_s"], md.get("le", (0.0, 0.0, 0.0)))
        hs = shell_half_size(k, n)
        p, tri = _box_mesh((-hs, -hs, -hs), (hs, hs, hs))
        b.create_instance(b.add_mesh("shell%d" % k, p, tri, mid))
        ids.append(mid)
    _floor(b, -0.1, floor_half)
    b.add_point_light((0.0, 0.05, 0.0), (1.0, 1.0, 1.0), 100.0)
    b.set_background(BACKGROUND)
    return b.build(), dict(pos=(0.0, 2.5, 7.0), at=(0.0, 0.0, 0.0), vfov=40.0), ids


SLAB_DENSE = dict(g=0.0, sigma_a=0.1, sigma_s=0.4)


def slab_row(m, medium=None, thickness=0.05, pitch=0.1):
    """m separate Volume slabs (z in [0.5 + pitch j, 0.5 + pitch j + thickness], +-3 wide) between a diffuse wall at z = 0 and a
    point light behind the last slab.  The camera stands between the wall and the first slab and looks at the wall: its rays meet no
    medium, the wall's connections cross 2 m boundaries.  medium: dict g, sigma_a, sigma_s (default: `thin`, so that the rays that
    bounce off the wall into the slabs make no event and no connection of their own).  -> (scene, camera dict, the slabs' material id)."""
    from aten_amd.scene.builder import SceneBuilder
    from aten_amd.scene.scenedefs import _box_mesh
    b = SceneBuilder()
    md = medium or thin(0)
    mid = b.add_medium_material("slab", md["g"], md["sigma_a"], md["sigma_s"])
    for j in range(m):
        z0 = 0.5 + pitch * j
        p, tri = _box_mesh((-3.0, -3.0, z0), (3.0, 3.0, z0 + thickness))
        b.create_instance(b.add_mesh("slab%d" % j, p, tri, mid))
    wall = b.add_material("wall", L.MTRL_DIFFUSE, (0.7, 0.7, 0.7))
    p = np.array([[-2, -2, 0], [2, -2, 0], [2, 2, 0], [-2, 2, 0]], F32)
    b.create_instance(b.add_mesh("wall", p, [[0, 1, 2], [0, 2, 3]], wall))       # the normal is +z
    b.add_point_light((0.0, 0.0, 0.5 + pitch * m + 0.5), (1.0, 1.0, 1.0), 100.0)
    b.set_background(BACKGROUND)
    return b.build(), dict(pos=(0.0, 0.0, 0.45), at=(0.0, 0.0, 0.0), vfov=60.0), mid


def node_image_bounds(fs):
    """(least, most) bytes of the scene's node image: a record is 32 or 48 bytes.  Above 32 KB the context walks global memory
    whatever ATEN_AMD_LDS_NODES says."""
    n = sum(len(l) for l in fs.arrays["bvh_lists"])
    return 32 * n, 48 * n


def walks_for(fs):
    """The walks a scene is run under: the context's own choice (the LDS copy while the node image fits 32 KB), the lane-refilling
    walk (ATEN_AMD_TRACE=r) and the plain walk over global memory (ATEN_AMD_LDS_NODES=0).  Where the image cannot fit, the context's
    own choice IS the plain global walk: the two global walks only."""
    return ("refill", "global") if node_image_bounds(fs)[0] > 32768 else ("own", "refill", "global")


def twin_stages(vq, scene, cam, seeds, w, h, frame, iterations=range(ITERATIONS), **kw):
    """The twin's captures of one frame after each iteration -> (list of stage dicts, the frame's counters)."""
    out, counters = [], None
    for k in iterations:
        v = vq.Volume()
        _, st = v.render(scene, cam, seeds, w, h, frame=frame, capture=k, **kw)
        out.append(st)
        counters = v.counters
    return out, counters


def pass_only(st):
    s = st["state"]
    return s["processed"] & s["passed"] & ~s["scattered"] & ~s["absorbed"]


def first_decision_masks(stages_by_iteration):
    """mask[k]: the pixels processed at iteration k that at every earlier iteration passed a boundary and neither scattered nor were
    absorbed.  Their inputs at k are bit-equal on the twin and the device (module docstring); mask[0] is every pixel."""
    masks = []
    so_far = np.ones_like(stages_by_iteration[0]["state"]["processed"])
    for st in stages_by_iteration:
        masks.append(so_far & st["state"]["processed"])
        so_far = so_far & pass_only(st)
    return masks


def events(st):
    return st["state"]["scattered"] | st["state"]["absorbed"]


def ulp_diff(a, b):
    a = np.ascontiguousarray(a, F32); b = np.ascontiguousarray(b, F32)
    ia = a.view(np.int32).astype(np.int64); ib = b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, np.int64(-2**31) - ia, ia)
    ib = np.where(ib < 0, np.int64(-2**31) - ib, ib)
    return np.abs(ia - ib)


def near_ties(st, mask):
    """The pixels of `mask` that sampled a distance within NEAR_TIE_ULPS of the hit distance."""
    m = mask & st["state"]["sampled"]
    out = np.zeros_like(m)
    out[m] = ulp_diff(st["ray"]["s"][m], st["ray"]["hit_t"][m]) <= NEAR_TIE_ULPS
    return out


def shells_by_hand(org, dirs, ids, n, floor_y=-0.1):
    """Hand-worked, without the twin's walk or stack code.  A straight ray through n concentric boxes enters shells 0 .. j-1 and
    then leaves them j-1 .. 0; the floor may cut the sequence short.  In float64, per ray: `passes`, the boundaries crossed before
    the floor (or all of them), and `stacks` [rays, 8 iterations, 8], `sizes` [rays, 8]: the stack after pass k + 1 -- the ids of the
    shells entered, in entry order, at most eight (a ninth push is dropped), shortened from the newest end on the way out; and `clear`:
    no two of the ray's meetings (boundaries, the floor) lie within 1e-3 of each other -- where they do (a ray through a box edge, a
    boundary that meets the floor under the ray) float32 may take them in the other order, and the hand has nothing to say."""
    org = np.asarray(org, np.float64).reshape(-1, 3)
    dirs = np.asarray(dirs, np.float64).reshape(-1, 3)
    nr = len(org)
    passes = np.zeros(nr, np.int32)
    stacks = np.zeros((nr, ITERATIONS, ITERATIONS), np.int32)
    sizes = np.zeros((nr, ITERATIONS), np.int32)
    clear = np.ones(nr, bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        t_floor = np.where(dirs[:, 1] < 0, (floor_y - org[:, 1]) / dirs[:, 1], np.inf)
        inv = 1.0 / dirs
    for i in range(nr):
        crossings = []
        for k in range(n):
            hs = shell_half_size(k, n)
            t0 = (-hs - org[i]) * inv[i]
            t1 = (hs - org[i]) * inv[i]
            tin, tout = np.minimum(t0, t1).max(), np.maximum(t0, t1).min()
            if tin < tout and tin > 0:
                crossings += [(tin, +1, k), (tout, -1, k)]
        ts = np.sort([c[0] for c in crossings] + [t_floor[i]])
        clear[i] = len(ts) < 2 or np.diff(ts).min() > 1e-3
        crossings = [c for c in sorted(crossings) if c[0] < t_floor[i]]
        passes[i] = len(crossings)
        st = []
        for k, (_, way, shell) in enumerate(crossings[:ITERATIONS]):
            if way > 0:
                if len(st) < ITERATIONS:
                    st.append(ids[shell])
            elif st:
                st.pop()
            sizes[i, k] = len(st)
            stacks[i, k, :len(st)] = st
    return passes, stacks, sizes, clear


_cache = {}


def case(orc, vq, name, n, w, h, frame, **kw):
    """One (scene, size, frame) of the gate, built and run on the twin once per session: dict scene, cam (the oracle's camera),
    seeds, ids, stages (the twin's captures at iterations 0 .. 7), masks, counters.  Nothing in it is written afterwards."""
    key = (name, n, w, h, frame, tuple(sorted(kw.items())))
    if key not in _cache:
        if name in ("slab_row", "slab_row_dense"):
            scene, cam, ids = slab_row(n, SLAB_DENSE if name == "slab_row_dense" else None)
        else:
            scene, cam, ids = nested_shells(n, name)
        c = orc.create_camera(cam["pos"], cam["at"], cam["vfov"], w, h)
        seeds = orc.init_sampler(w, h, 0)
        stages, counters = twin_stages(vq, scene, c, seeds, w, h, frame, **kw)
        _cache[key] = dict(scene=scene, cam=c, seeds=seeds, ids=ids, stages=stages, masks=first_decision_masks(stages), counters=counters)
    return _cache[key]
