"""Shadow-ray sets for the per-ray visibility gate (tests/test_shadow_oracle_cpu.py, tests/test_gpu_shadow_rays.py).

Every builder is deterministic (seeded) and builds its rays from the ORACLE's own closest hits, so the geometry each ray meets is known:
  A  surface-born rays: ray_offset(p, n) at primary hits of a 64 x 36 frame and at the hits of one hemisphere bounce, towards every light
  B  distance straddle: a ray through the interior of a known blocker at t_hit, distToLight stepped around t_hit (point / spot lights)
  C  lamp geometry: targets on the lamp's interior, edges, diagonal and just outside its rim, back-side and grazing rays, origins close
     enough to flip the planar certificate's offset bound
  D  ignored surfaces: rays through alpha panes / stencil surfaces, each with the stencil flag off and on
  E  shape edges: unnormalised and axis-parallel directions, +0.0 / -0.0 components, the last light index
A RaySet keeps a category label per ray.  `restate_opaque` is scene::hitLight written in NumPy over orc.trace_closest; `pane_stack`
and `pane_stack_verdict` are the stack scene and its verdict by counting panes against the lookup budget."""
import numpy as np

from aten_amd import layout as L

F32 = np.float32
EPS = F32(1e-9)         # AT_MATH_EPSILON
FLOOR = 0.05            # neither verdict may fall under this share of a category's rays


def normalize32(v):
    """aten::normalize in float32: v * (1 / sqrt((x x + y y) + z z)), every operation rounded on its own."""
    v = np.ascontiguousarray(v, F32).reshape(-1, 3)
    s = v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]
    s = s + v[:, 2] * v[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        return v * (F32(1.0) / np.sqrt(s))[:, None]


def length32(v):
    v = np.ascontiguousarray(v, F32).reshape(-1, 3)
    s = v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]
    return np.sqrt(s + v[:, 2] * v[:, 2])


class RaySet:
    def __init__(self, org, dirs, dist, light, cat, stencil=False):
        self.org = np.ascontiguousarray(org, F32).reshape(-1, 3)
        n = len(self.org)
        self.dir = np.ascontiguousarray(np.broadcast_to(np.asarray(dirs, F32), (n, 3)))
        self.dist = np.ascontiguousarray(np.broadcast_to(np.asarray(dist, F32), (n,)))
        self.light = np.ascontiguousarray(np.broadcast_to(np.asarray(light, np.int32), (n,)))
        self.stencil = np.ascontiguousarray(np.broadcast_to(np.asarray(stencil, bool), (n,)))
        self.cat = np.ascontiguousarray(np.broadcast_to(np.asarray(cat, "U24"), (n,)))

    def __len__(self):
        return len(self.org)

    def take(self, idx):
        return RaySet(self.org[idx], self.dir[idx], self.dist[idx], self.light[idx], self.cat[idx], self.stencil[idx])

    def with_stencil(self, on):
        return RaySet(self.org, self.dir, self.dist, self.light, self.cat, on)

    def relabel(self, cat):
        return RaySet(self.org, self.dir, self.dist, self.light, cat, self.stencil)

    @staticmethod
    def concat(sets):
        sets = [s for s in sets if len(s)]
        return RaySet(*[np.concatenate([getattr(s, k) for s in sets]) for k in ("org", "dir", "dist", "light", "cat", "stencil")])

    def queries(self, orc):
        return orc.shadow_queries(self.org, self.dir, self.dist, self.light, self.stencil)


def check_floor(rs, visible, what=""):
    """Both verdicts occur in at least FLOOR of every category's rays (first letter of the label = the category)."""
    letters = np.array([c[0] for c in rs.cat])
    for c in np.unique(letters):
        share = float(np.asarray(visible, bool)[letters == c].mean())
        assert FLOOR <= share <= 1.0 - FLOOR, "%s category %s: %.3f of %d rays visible" % (what, c, share, int((letters == c).sum()))


def mismatch_report(rs, got, want, limit=12):
    """The first mismatching queries with their category, and the mismatch count per category."""
    bad = np.flatnonzero(np.asarray(got) != np.asarray(want))
    lines = ["%d of %d verdicts differ" % (len(bad), len(rs))]
    for c in np.unique(rs.cat[bad]):
        lines.append("  %-24s %d of %d" % (c, int((rs.cat[bad] == c).sum()), int((rs.cat == c).sum())))
    for i in bad[:limit]:
        lines.append("  #%d [%s] org=%r dir=%r dist=%r light=%d stencil=%d: got %d, oracle %d"
                     % (i, rs.cat[i], rs.org[i].tolist(), rs.dir[i].tolist(), float(rs.dist[i]), rs.light[i], rs.stencil[i], got[i], want[i]))
    return "\n".join(lines)


# ---- scene::hitLight over the oracle's closest hits (opaque scenes) -----------------------------------------------------------------
def restate_opaque(orc, fs, rs):
    """HitTestToTargetLight where no surface can be ignored (one lookup): closest hit of Ray(org, normalize(dir)) in [EPS, dist - EPS],
    then  no hit or the light's own object -> visible;  infinite light -> !hit;  singular light -> t > dist;  otherwise blocked."""
    rays = np.zeros(len(rs), L.RAY)
    rays["org"] = rs.org
    rays["dir"] = normalize32(rs.dir)
    hits = np.zeros(len(rs), L.INTERSECTION)
    bits = rs.dist.view(np.uint32)
    order = np.argsort(bits, kind="stable")
    cuts = np.flatnonzero(np.diff(bits[order])) + 1
    for idx in np.split(order, cuts):       # (orc.trace_closest takes one t_max per call)
        d = rs.dist[idx[0]]
        hits[idx] = orc.trace_closest(fs, rays[idx], float(EPS), float(F32(d - EPS)))[0]
    lights = fs.arrays["lights"][rs.light]
    is_hit = hits["objid"] >= 0
    lightobj = np.where((lights["type"] == L.LIGHT_AREA) & (lights["arealight_objid"] >= 0), lights["arealight_objid"], -1)
    same = np.where(is_hit, hits["objid"] == lightobj, True)
    infinite = (lights["attrib"] & L.LATTR_INFINITE) != 0
    singular = (lights["attrib"] & L.LATTR_SINGULAR) != 0
    with np.errstate(invalid="ignore"):
        vis = np.where(same, True, np.where(infinite, ~is_hit, np.where(singular, hits["t"] > rs.dist, False)))
    return vis.astype(np.uint8), hits


# ---- geometry from the oracle's hits -----------------------------------------------------------------------------------------------
def surface_points(orc, fs, cam, w=64, h=36, seed=7):
    """(p, n): the primary hits of a w x h frame and the hits of one random hemisphere bounce from them; n faces the arriving ray."""
    c = orc.create_camera(cam["pos"], cam["at"], cam["vfov"], w, h)
    rays = orc.generate_paths(c, orc.init_sampler(w, h, 0), w, h, 0, 0)
    rng = np.random.default_rng(seed)
    out_p, out_n = [], []
    for bounce in range(2):
        hit, _ = orc.trace_closest(fs, rays)
        ok = hit["objid"] >= 0
        ev = orc.evaluate_hits(fs, rays, hit)
        p, n, d = ev[ok, 0:3], ev[ok, 4:7], rays["dir"][ok]
        n = np.where(((n * d).sum(-1) > 0)[:, None], -n, n).astype(F32)
        good = np.isfinite(p).all(-1) & np.isfinite(n).all(-1) & (np.abs(length32(n) - 1.0) < 1e-3)
        p, n = p[good], n[good]
        out_p.append(p); out_n.append(n)
        v = rng.normal(size=(len(p), 3)).astype(F32)
        v = normalize32(v)
        v = np.where(((v * n).sum(-1) < 0)[:, None], -v, v).astype(F32)
        rays = np.zeros(len(p), L.RAY)
        rays["org"] = orc.ray_offset(p, n)
        rays["dir"] = v
    return np.concatenate(out_p), np.concatenate(out_n)


def lamp_triangles(fs, light):
    """World-space triangles [T, 3, 3] (float64) of an area light's polygon object, or None (sphere, or no object)."""
    a = fs.arrays
    oid = int(a["lights"][light]["arealight_objid"])
    if int(a["lights"][light]["type"]) != L.LIGHT_AREA or oid < 0:
        return None
    o = a["objects"][oid]
    M = np.eye(4)
    if int(o["type"]) == L.OBJ_INSTANCE:
        M = a["matrices"][int(o["mtx_id"])].astype(np.float64)
        o = a["objects"][int(o["object_id"])]
    if int(o["type"]) != L.OBJ_POLYGONS:
        return None
    t0, tn = int(o["triangle_id"]), int(o["triangle_num"])
    v = a["vtx_pos"][a["triangles"]["idx"][t0:t0 + tn].reshape(-1), :3].astype(np.float64)
    return (v @ M[:3, :3].T + M[:3, 3]).reshape(tn, 3, 3)


def scene_extent(fs):
    v = fs.arrays["vtx_pos"][:, :3]
    return float(np.linalg.norm(v.max(0) - v.min(0)))


def light_targets(fs, light, p, rng):
    """What FillShadowRay stores for a sample of `light` seen from p: (normalised direction, distToLight)."""
    a = fs.arrays
    l = a["lights"][light]
    p = np.ascontiguousarray(p, F32)
    kind = int(l["type"])
    if kind == L.LIGHT_DIRECTION:
        d = -normalize32(np.tile(l["dir"][:3], (len(p), 1)))
        dist = np.full(len(p), 50000.0, F32)        # |pos - p| of Light_sample's pos = p + 100000 * 0.5 * dir
        dist[::4] = np.inf                          # (and the unbounded form)
        return d, dist
    if kind == L.LIGHT_IBL:
        d = normalize32(rng.normal(size=(len(p), 3)))
        return d, np.full(len(p), 2.0 * scene_extent(fs), F32)
    if kind == L.LIGHT_AREA:
        tris = lamp_triangles(fs, light)
        if tris is None:        # a sphere lamp: points on the sphere
            o = a["objects"][int(l["arealight_objid"])]
            if int(o["type"]) == L.OBJ_INSTANCE:
                o = a["objects"][int(o["object_id"])]
            pos = o["sphere_center"] + o["sphere_radius"] * normalize32(rng.normal(size=(len(p), 3)))
        else:
            t = tris[rng.integers(0, len(tris), len(p))]
            u, v = rng.random(len(p)), rng.random(len(p))
            flip = u + v > 1
            u, v = np.where(flip, 1 - u, u), np.where(flip, 1 - v, v)
            pos = t[:, 0] + u[:, None] * (t[:, 1] - t[:, 0]) + v[:, None] * (t[:, 2] - t[:, 0])
        pos = pos.astype(F32)
    else:
        pos = np.tile(l["pos"][:3], (len(p), 1)).astype(F32)
    d = (pos - p).astype(F32)
    return normalize32(d), length32(d)


# ---- A ---------------------------------------------------------------------------------------------------------------------------
def category_a(orc, fs, pts, seed=11, limit=6000):
    """Surface-born rays: light k % n_lights for point k (every light, the last one included)."""
    p, n = pts
    rng = np.random.default_rng(seed)
    if len(p) > limit:
        keep = np.sort(rng.choice(len(p), limit, replace=False))
        p, n = p[keep], n[keep]
    n_lights = len(fs.arrays["lights"])
    org = orc.ray_offset(p, n)
    sets = []
    for li in range(n_lights):
        sel = np.arange(len(p)) % n_lights == li
        d, dist = light_targets(fs, li, p[sel], rng)
        sets.append(RaySet(org[sel], d, dist, li, "A surface-born"))
    return RaySet.concat(sets)


# ---- B ---------------------------------------------------------------------------------------------------------------------------
def _step_ulps(x, k):
    return (x.view(np.int32) + np.int32(k)).view(F32)


def category_b(orc, fs, pts, seed=13, limit=400):
    """Rays from surface points towards each point / spot light that pass through the INTERIOR of a blocker (barycentrics at least
    0.05 from every edge) at t_hit; distToLight = t_hit, t_hit +-1, +-2, +-64 ulps, t_hit +- EPS, +- 2 EPS, 0, and EPS / 2 (t_max < 0)."""
    p, n = pts
    a = fs.arrays
    org = orc.ray_offset(p, n)
    sets = []
    for li, l in enumerate(a["lights"]):
        if int(l["type"]) not in (L.LIGHT_POINT, L.LIGHT_SPOT):
            continue
        d = normalize32(np.tile(l["pos"][:3], (len(p), 1)).astype(F32) - p)
        rays = np.zeros(len(p), L.RAY)
        rays["org"], rays["dir"] = org, d
        hit, _ = orc.trace_closest(fs, rays)
        to_light = length32(np.tile(l["pos"][:3], (len(p), 1)).astype(F32) - p)
        ok = (hit["objid"] >= 0) & (hit["a"] > 0.05) & (hit["b"] > 0.05) & (hit["a"] + hit["b"] < 0.95) & (hit["t"] > 1e-2) & (hit["t"] < to_light)
        idx = np.flatnonzero(ok)[:limit]
        t = np.ascontiguousarray(hit["t"][idx], F32)
        steps = [("t_hit", t)]
        for k in (1, 2, 64):
            steps.append(("t_hit+%dulp" % k, _step_ulps(t, k)))
            steps.append(("t_hit-%dulp" % k, _step_ulps(t, -k)))
        for k in (1, 2):
            steps.append(("t_hit+%dEPS" % k, (t + F32(k) * EPS).astype(F32)))
            steps.append(("t_hit-%dEPS" % k, (t - F32(k) * EPS).astype(F32)))
        steps.append(("zero", np.zeros_like(t)))
        steps.append(("below EPS", np.full_like(t, 0.5e-9)))
        for name, dist in steps:
            sets.append(RaySet(org[idx], d[idx], dist, li, "B " + name))
    return RaySet.concat(sets)


# ---- C ---------------------------------------------------------------------------------------------------------------------------
def category_c(orc, fs, light, pts, seed=17, per=300):
    """Rays about the area lamp `light` (a planar polygon): see the module docstring.  Origins are surface points (through ray_offset)
    unless the sub-category places them itself."""
    rng = np.random.default_rng(seed)
    tris = lamp_triangles(fs, light)
    p, n = pts
    org_all = orc.ray_offset(p, n)
    nrm = np.cross(tris[0, 1] - tris[0, 0], tris[0, 2] - tris[0, 0])
    nrm /= np.linalg.norm(nrm)
    centre = tris.reshape(-1, 3).mean(0)
    front = nrm if np.dot(np.median(p, 0) - centre, nrm) > 0 else -nrm       # the side the scene's surfaces are on
    # edges: those that occur once are the rim, the one that occurs twice is the shared diagonal
    edges = {}
    for t in tris:
        for i in range(3):
            key = tuple(sorted([tuple(np.round(t[i], 6)), tuple(np.round(t[(i + 1) % 3], 6))]))
            edges.setdefault(key, []).append((t[i], t[(i + 1) % 3]))
    rim = [v[0] for v in edges.values() if len(v) == 1]
    diag = [v[0] for v in edges.values() if len(v) == 2]

    def on_edges(es, k):
        e = [es[i] for i in rng.integers(0, len(es), k)]
        s = rng.uniform(0.02, 0.98, k)
        a0 = np.array([x[0] for x in e]); a1 = np.array([x[1] for x in e])
        pos = a0 + s[:, None] * (a1 - a0)
        out = np.cross(a1 - a0, nrm)
        out /= np.linalg.norm(out, axis=1)[:, None]
        out *= np.sign(((pos - centre) * out).sum(-1))[:, None]
        return pos, out

    def interior(k):
        t = tris[rng.integers(0, len(tris), k)]
        u, v = rng.uniform(0.05, 0.9, k), rng.uniform(0.05, 0.9, k)
        flip = u + v > 0.95
        u, v = np.where(flip, 0.95 - u, u), np.where(flip, 0.95 - v, v)
        return t[:, 0] + u[:, None] * (t[:, 1] - t[:, 0]) + v[:, None] * (t[:, 2] - t[:, 0])

    def from_surface(pos, cat):
        k = len(pos)
        sel = rng.integers(0, len(p), k)
        d = (pos.astype(F32) - p[sel]).astype(F32)
        return RaySet(org_all[sel], normalize32(d), length32(d), light, cat)

    def from_origin(o, pos, cat):
        o = o.astype(F32)
        d = (pos.astype(F32) - o).astype(F32)
        return RaySet(o, normalize32(d), length32(d), light, cat)

    sets = [from_surface(interior(4 * per), "C interior")]
    sets.append(from_surface(on_edges(rim, per)[0], "C rim edge"))
    if diag:
        sets.append(from_surface(on_edges(diag, per)[0], "C diagonal"))
    for eps in (1e-4, -1e-4):
        pos, out = on_edges(rim, per)
        sets.append(from_surface(pos + eps * out, "C rim %+.0e" % eps))
    # from the lamp's back side
    pos = interior(per)
    lateral = rng.normal(size=(per, 3)) * 0.2
    lateral -= (lateral @ nrm)[:, None] * nrm
    sets.append(from_origin(pos - front * rng.uniform(0.01, 0.5, per)[:, None] + lateral, pos, "C back side"))
    # grazing: the angle between the ray and the lamp's plane has sine cos_l
    for cos_l in (0.009, 0.0100, 0.011):
        pos = interior(per)
        u = rng.normal(size=(per, 3))
        u -= (u @ nrm)[:, None] * nrm
        u /= np.linalg.norm(u, axis=1)[:, None]
        r = rng.uniform(0.3, 1.5, per)[:, None]
        sets.append(from_origin(pos + r * (u * np.sqrt(1 - cos_l ** 2) + front * cos_l), pos, "C grazing %.4f" % cos_l))
    # origins close to the lamp: the certificate's offset bound (off <= 5e-4 dist cos_l) flips with the distance
    for dist in (0.02, 0.05, 0.1, 0.2, 0.24, 0.26, 0.3, 0.5):
        pos = interior(per // 4)
        lateral = rng.normal(size=(len(pos), 3)) * 0.3 * dist
        lateral -= (lateral @ nrm)[:, None] * nrm
        sets.append(from_origin(pos + front * dist + lateral, pos, "C near %.2f" % dist))
    return RaySet.concat(sets)


# ---- D: the pane stack -------------------------------------------------------------------------------------------------------------
PANE_Y0, PANE_DY, PANE_HALF, PANE_CELLS = 0.4, 0.05, 0.8, 8
STRIP_Y, STRIP_X0, STRIP_X1 = 1.2, 0.15, 0.5       # the opaque strip above the panes (z in -1 .. 1): it shades part of the stack


def pane_stack(k, blending, lamp=False):
    """k parallel alpha-textured panes (an 8 x 8 checker, alpha 0.4 / 1.0) between a floor and a point light; an opaque strip above the
    panes shades part of them.  lamp=True: the light is an area lamp whose material has alpha 0.5 -- a shadow ray that reaches it ignores it
    and misses behind it."""
    from aten_amd.scene.builder import SceneBuilder
    b = SceneBuilder()
    white = b.add_material("white", L.MTRL_DIFFUSE, (0.7, 0.7, 0.7))
    tex = np.ones((PANE_CELLS, PANE_CELLS, 4), F32)
    tex[..., :3] = 0.9
    tex[(np.add.outer(np.arange(PANE_CELLS), np.arange(PANE_CELLS)) % 2) == 0, 3] = 0.4
    pane = b.add_material("pane", L.MTRL_DIFFUSE, (1.0, 1.0, 1.0, 1.0), albedo_map=b.add_texture("alpha_checker", tex))
    uv = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], F32)

    def quad(name, y, x0, x1, z0, z1, mtrl, uvs=None, flip=False):
        q = np.array([[x0, y, z0], [x1, y, z0], [x1, y, z1], [x0, y, z1]], F32)
        idx = [[0, 2, 1], [0, 3, 2]] if flip else [[0, 1, 2], [0, 2, 3]]
        return b.create_instance(b.add_mesh(name, q, idx, mtrl, uvs=uvs))

    quad("floor", 0.0, -2.0, 2.0, -2.0, 2.0, white, flip=True)
    for j in range(k):
        quad("pane%d" % j, PANE_Y0 + PANE_DY * j, -PANE_HALF, PANE_HALF, -PANE_HALF, PANE_HALF, pane, uvs=uv)
    quad("strip", STRIP_Y, STRIP_X0, STRIP_X1, -1.0, 1.0, white)
    if lamp:
        emit = b.add_material("lamp", L.MTRL_EMISSIVE, (1.0, 1.0, 1.0, 0.5))
        b.add_area_light(quad("lamp", 2.0, -0.3, 0.3, -0.3, 0.3, emit), (1.0, 1.0, 1.0), 30.0)
    else:
        b.add_point_light((0.0, 2.0, 0.0), (1.0, 0.9, 0.8), 30.0)
    b.config.enable_alpha_blending = 1 if blending else 0
    b.set_background((0.1, 0.15, 0.2))
    return b.build(), dict(pos=(0.0, 1.0, 4.0), at=(0.0, 0.8, 0.0), vfov=45.0)


def category_d_stack(orc, fs, seed=19, n=1500):
    """Rays from the floor (ray_offset of points on it) to the light -- the point light, or random points on the lamp --, each with the
    stencil flag off and on.  Origins are kept only where every pane crossing lies at least a tenth of a cell inside its checker cell
    and 0.02 away from the strip's and the panes' borders, so that counting panes is not a matter of rounding."""
    rng = np.random.default_rng(seed)
    p = np.zeros((16 * n, 3), F32)
    p[:, 0], p[:, 2] = rng.uniform(-1.6, 1.6, len(p)), rng.uniform(-1.6, 1.6, len(p))
    nrm = np.tile(np.array([0, 1, 0], F32), (len(p), 1))
    d, dist = light_targets(fs, 0, p, rng)
    target = p + d * dist[:, None]
    keep = np.ones(len(p), bool)
    for y, half, cells in [(PANE_Y0 + PANE_DY * j, PANE_HALF, PANE_CELLS) for j in range(pane_count(fs))] + [(STRIP_Y, None, 0)]:
        s = (y - p[:, 1]) / (target[:, 1] - p[:, 1])
        x = p[:, 0] + s * (target[:, 0] - p[:, 0]); z = p[:, 2] + s * (target[:, 2] - p[:, 2])
        if half is None:
            keep &= (np.abs(x - STRIP_X0) > 0.02) & (np.abs(x - STRIP_X1) > 0.02) & (np.abs(np.abs(z) - 1.0) > 0.02)
            continue
        keep &= (np.abs(np.abs(x) - half) > 0.02) & (np.abs(np.abs(z) - half) > 0.02)
        inside = (np.abs(x) < half) & (np.abs(z) < half)
        for c in (x, z):
            f = (c + half) / (2 * half) * cells
            keep &= ~inside | (np.abs(f - np.round(f)) > 0.1)
    idx = np.flatnonzero(keep)[:n]
    base = RaySet(orc.ray_offset(p[idx], nrm[idx]), d[idx], dist[idx], 0, "D stack")
    return RaySet.concat([base.with_stencil(False).relabel("D stack flag off"), base.with_stencil(True).relabel("D stack flag on")])


def pane_count(fs):
    # floor, strip, the light's quad if any: every other instance is a pane
    a = fs.arrays
    n_inst = int((a["objects"]["type"] == L.OBJ_INSTANCE).sum())
    return n_inst - 2 - (1 if int(a["lights"][0]["type"]) == L.LIGHT_AREA else 0)


def pane_stack_verdict(orc, fs, rs, blending):
    """The stack's verdict by counting: the panes a ray crosses in order, then the strip; an opaque texel or the strip blocks; every
    translucent pane (and the alpha lamp, if it is the target) costs a lookup, and the light is reached only if a lookup is left for the
    final miss.  Returns (visible, decided): rays of the lamp scene that cross no pane meet the lamp AT distToLight -- a rounding
    decides whether the walk finds it -- and are left undecided."""
    k = pane_count(fs)
    lamp = int(fs.arrays["lights"][0]["type"]) == L.LIGHT_AREA
    o = rs.org.astype(np.float64); d = normalize32(rs.dir).astype(np.float64)
    budget = np.where(rs.stencil | bool(blending), 10, 1)
    ignored = np.zeros(len(rs), np.int64)
    blocked = np.zeros(len(rs), bool)
    for j in range(k):
        s = (PANE_Y0 + PANE_DY * j - o[:, 1]) / d[:, 1]
        x, z = o[:, 0] + s * d[:, 0], o[:, 2] + s * d[:, 2]
        inside = (np.abs(x) < PANE_HALF) & (np.abs(z) < PANE_HALF) & (s < rs.dist)
        uv = np.stack([(x + PANE_HALF) / (2 * PANE_HALF), (z + PANE_HALF) / (2 * PANE_HALF)], -1)
        alpha = orc.sample_texture(fs, 0, uv.astype(F32))[:, 3]
        live = inside & ~blocked
        blocked |= live & (alpha >= 1.0)
        ignored += live & (alpha < 1.0)
    s = (STRIP_Y - o[:, 1]) / d[:, 1]
    x, z = o[:, 0] + s * d[:, 0], o[:, 2] + s * d[:, 2]
    blocked |= (x > STRIP_X0) & (x < STRIP_X1) & (np.abs(z) < 1.0) & (s < rs.dist)
    lookups = ignored + (1 if lamp else 0) + 1          # the ignored hits, the ignored lamp, the final miss
    visible = ~blocked & (lookups <= budget)
    decided = np.ones(len(rs), bool) if not lamp else (blocked | (ignored > 0))
    return visible.astype(np.uint8), decided


def category_d_room(orc, fs, pts, seed=23, limit=2500):
    """The stencil / alpha room: surface-born rays towards its light, each with the stencil flag off and on."""
    base = category_a(orc, fs, pts, seed=seed, limit=limit)
    return RaySet.concat([base.with_stencil(False).relabel("D room flag off"), base.with_stencil(True).relabel("D room flag on")])


# ---- E ---------------------------------------------------------------------------------------------------------------------------
def category_e(orc, fs, pts, seed=29, per=350):
    """Unnormalised directions (length 0.5 and 3) towards the lights, axis-parallel directions whose other components are exactly +0.0
    and -0.0, all towards the LAST light index (and, for the scaled ones, every light)."""
    p, n = pts
    rng = np.random.default_rng(seed)
    sel = np.sort(rng.choice(len(p), min(len(p), 2 * per), replace=False))
    a = category_a(orc, fs, (p[sel], n[sel]), seed=seed)
    sets = [RaySet(a.org, (a.dir * F32(s)).astype(F32), a.dist, a.light, "E length %g" % s) for s in (0.5, 3.0)]
    last = len(fs.arrays["lights"]) - 1
    l = fs.arrays["lights"][last]
    infinite = (int(l["attrib"]) & L.LATTR_INFINITE) != 0
    org = orc.ray_offset(p, n)
    ext = scene_extent(fs)
    for axis in range(3):
        for sign in (1.0, -1.0):
            for zero in (0.0, -0.0):
                d = np.full(3, zero, F32)
                d[axis] = sign
                # leave the surface: only points whose normal has a component along the direction
                ok = np.flatnonzero(n[:, axis] * sign > 0.3)
                if len(ok) == 0:
                    continue
                idx = ok[rng.integers(0, len(ok), per // 6)]
                dist = np.full(len(idx), 50000.0, F32) if infinite else rng.uniform(0.05, 0.5, len(idx)).astype(F32) * F32(ext)
                sets.append(RaySet(org[idx], d, dist, last, "E axis %s%s zero %s" % ("+" if sign > 0 else "-", "xyz"[axis], "+0" if np.signbit(zero) == 0 else "-0")))
    return RaySet.concat(sets)


E_SIZES = [1, 63, 64, 65, 1023, 1024, 1025, 4099]


# ---- the cases: scene -> (FlatScene, camera, RaySet), built once per session ---------------------------------------------------------
def _room(light, blending):
    from test_gpu_shadow_plain import _stencil_alpha_room
    fs, cam = _stencil_alpha_room(light)
    fs.desc.config.enable_alpha_blending = 1 if blending else 0
    return fs, cam


def _hostile(offset):
    from test_gpu_anyhit_twin import _hostile_lamp_scene
    return _hostile_lamp_scene((offset, offset, offset))


def _variant(lights):
    from aten_amd.scene import scenedefs
    return scenedefs.cornell_box_variant(lights=lights)


def _sponza_with_point(sponza=None):
    from aten_amd.scene import scenedefs
    return scenedefs.sponza_lod(add_lights=lambda b, lo, hi, cam: b.add_point_light((0.0, 1.5, 0.0), (1.0, 0.9, 0.8), 20.0))


def _atrium():
    from aten_amd.scene import scenedefs
    return scenedefs.atrium(detail=0.25)


# name -> (scene factory, categories, the scene has no surface a shadow ray can ignore)
CASES = {"cornell": (None, "ACE", True)}          # (the session's `cornell` fixture)
for _k in ("point", "spot", "mixed"):
    CASES[_k] = ((lambda k=_k: _variant(k)), "ABE", True)
for _k in ("directional", "sphere"):
    CASES[_k] = ((lambda k=_k: _variant(k)), "AE", True)
CASES["hostile"] = ((lambda: _hostile(0.0)), "C", True)
CASES["hostile_1e4"] = ((lambda: _hostile(1e4)), "C", True)
for _l in ("point", "directional"):
    for _b in (1, 0):
        CASES["room_%s_%s" % (_l, "blend" if _b else "noblend")] = ((lambda l=_l, b=_b: _room(l, b)), "D", False)
STACKS = []
for _lamp in (False, True):
    for _b in (1, 0):
        for _k in (1, 9, 10, 11):
            _name = "%s_k%d_%s" % ("lampstack" if _lamp else "stack", _k, "blend" if _b else "noblend")
            CASES[_name] = ((lambda k=_k, b=_b, lamp=_lamp: pane_stack(k, b, lamp)), "d", False)
            STACKS.append((_name, _k, _b, _lamp))
CASES["sponza"] = (_sponza_with_point, "AE", True)
CASES["atrium"] = (_atrium, "AE", True)
_cases = {}


def case(orc, name, cornell=None):
    """(FlatScene, camera, RaySet, the oracle's verdicts) of a case; every category's rays in one set."""
    if name not in _cases:
        make, cats, _ = CASES[name]
        fs, cam = cornell if make is None else make()
        sets = []
        if cats == "d":
            sets.append(category_d_stack(orc, fs))
        else:
            pts = surface_points(orc, fs, cam)
            if "A" in cats:
                sets.append(category_a(orc, fs, pts))
            if "B" in cats:
                sets.append(category_b(orc, fs, pts))
            if "C" in cats:
                sets.append(category_c(orc, fs, 0, pts))
            if "D" in cats:
                sets.append(category_d_room(orc, fs, pts))
            if "E" in cats:
                sets.append(category_e(orc, fs, pts))
        rs = RaySet.concat(sets)
        _cases[name] = (fs, cam, rs, orc.shadow_visible(fs, rs.queries(orc)))
    return _cases[name]
