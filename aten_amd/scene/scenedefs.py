"""Scene definitions for the BASELINE configs, following src/common/scenedefs.cpp of the reference.

  cornell_box()  <- ObjCornellBoxScene::makeScene / getCameraPosAndAt (scenedefs.cpp:732-802)
  sponza_lod()   <- SponzaScene (scenedefs.cpp:806-860) restricted to the blobs that exist:
                    asset/sponza/sponza_lod.obj + sponza_lod.sbvh (+ textures).  The full
                    sponza.obj/.sbvh are missing large blobs in the reference snapshot.
Data files are committed under assets/ (copied byte-for-byte from /root/reference/asset).
"""
import os

import numpy as np

from .. import layout as L
from .builder import SceneBuilder

ASSETS = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "assets")


def cornell_box(asset_dir=None):
    """Returns (FlatScene, camera dict(pos, at, vfov))."""
    asset_dir = asset_dir or os.path.join(ASSETS, "cornellbox")
    b = SceneBuilder()
    emit = b.add_material("light", L.MTRL_EMISSIVE, (1.0, 1.0, 1.0))      # scenedefs.cpp:735

    def create_mtrl(name, mtype, clr, albedo, nml):                        # scenedefs.cpp:738-771
        if name == "shortBox":
            return b.add_material(name, L.MTRL_SPECULAR, (0.7, 0.6, 0.5), roughness=0.1, ior=0.01)
        if name == "floor":
            return b.add_material(name, L.MTRL_GGX, (0.7, 0.6, 0.5), roughness=0.1, ior=0.01)
        return b.add_material(name, mtype, clr)

    objs = b.load_obj(os.path.join(asset_dir, "orig.obj"), create_mtrl=create_mtrl,
                      separate_objs=True, normal_on_the_fly=True)
    # createInstance(ctxt, objs[0], trans 0, rot 0, scale 1): identity matrix pair (:775-781)
    light = b.create_instance(objs[0])
    b.add_area_light(light, b.materials[emit][1]["baseColor"][:3], 200.0)  # :783-784
    for o in objs[1:]:
        b.create_instance(o)                                               # :786-789
    b.set_background((0.0, 0.0, 0.0))
    cam = dict(pos=(0.0, 1.0, 3.0), at=(0.0, 1.0, 0.0), vfov=45.0)         # :794-802
    return b.build(), cam


def synthetic_envmap(w=2048, h=1024, seed=0):
    """Stand-in for the missing asset/envmap/studio015.hdr: smooth analytic sky + sun lobe.

    value(u, v) = sky(v) + sun, with
      sky  = mix((0.35,0.30,0.25), (0.45,0.65,1.0), smoothstep(0.45,0.75,v)) * 1.2
      sun  = (60,55,45) * exp(-((u-0.3)^2 + (v-0.8)^2) / 0.0008)
    Stored in aten's texture order (row 0 = v near 0 = bottom).  `seed` is unused (kept so the
    fixture name records determinism).
    """
    v = (np.arange(h, dtype=np.float32) + 0.5) / h
    u = (np.arange(w, dtype=np.float32) + 0.5) / w
    t = np.clip((v - 0.45) / 0.3, 0, 1)
    t = t * t * (3 - 2 * t)
    ground = np.array([0.35, 0.30, 0.25], np.float32)
    sky = np.array([0.45, 0.65, 1.0], np.float32)
    col = (ground[None, :] * (1 - t[:, None]) + sky[None, :] * t[:, None]) * np.float32(1.2)
    img = np.repeat(col[:, None, :], w, axis=1)
    d2 = (u[None, :] - 0.3) ** 2 + (v[:, None] - 0.8) ** 2
    sun = np.exp(-d2 / 0.0008).astype(np.float32)
    img = img + sun[:, :, None] * np.array([60, 55, 45], np.float32)[None, None, :]
    out = np.ones((h, w, 4), np.float32)
    out[:, :, :3] = img
    return out


def envmap_avg_illum(tex):
    """ImageBasedLight::preCompute's sin(theta)-weighted mean luminance (light/ibl.cpp:10-75)."""
    h = tex.shape[0]
    lum = 0.212639 * tex[:, :, 0] + 0.71517 * tex[:, :, 1] + 0.0721926 * tex[:, :, 2]
    theta = np.pi * (np.arange(h) + 0.5) / h
    s = np.sin(theta)[:, None]
    return float((lum * s).sum() / (s.sum() * tex.shape[1]))


def sponza_lod(asset_dir=None, mtype=L.MTRL_GGX, ibl=True, use_sbvh=True, textures=True, bvh_options=None, optimize_sbvh=False,
               add_lights=None):
    """BASELINE config 3 stand-in: sponza_lod.obj (12,852 tris) with the reference-built
    sponza_lod.sbvh tree, GGX materials, synthetic IBL.  add_lights(builder, bbox_min, bbox_max, cam): extra lights."""
    asset_dir = asset_dir or os.path.join(ASSETS, "sponza")
    b = SceneBuilder()

    def create_mtrl(name, mt, clr, albedo, nml):
        alb = b.load_image(os.path.join(asset_dir, albedo)) if (albedo and textures) else -1
        nm = b.load_image(os.path.join(asset_dir, nml)) if (nml and textures) else -1
        if callable(mtype):         # mtype(builder, name, colour, albedo map, normal map) -> material id
            return mtype(b, name, clr, alb, nm)
        if mtype == L.MTRL_GGX:
            return b.add_material(name, L.MTRL_GGX, clr, albedo_map=alb, normal_map=nm, roughness=0.3, ior=0.01)
        if mtype == L.MTRL_DISNEY:
            return b.add_material(name, L.MTRL_DISNEY, clr, albedo_map=alb, normal_map=nm,
                                  roughness=0.4, metallic=0.1, specular=0.5, clearcoat=0.2)
        return b.add_material(name, mt, clr, albedo_map=alb, normal_map=nm)

    cam = dict(pos=(0.0, 1.0, 3.0), at=(0.0, 1.0, 0.0), vfov=45.0)         # scenedefs.cpp:847-860
    # own tree (use_sbvh=False): children nearer the viewer are threaded first
    b.bvh_options = dict(order_point=cam["pos"]) if bvh_options is None else bvh_options
    objs = b.load_obj(os.path.join(asset_dir, "sponza_lod.obj"), create_mtrl=create_mtrl)
    if use_sbvh:
        b.import_sbvh(objs[0], os.path.join(asset_dir, "sponza_lod.sbvh"), optimize=optimize_sbvh)
    b.create_instance(objs[0])
    if add_lights is not None:
        p = np.asarray(b.pos, np.float32).reshape(-1, 4)[:, :3]
        add_lights(b, p.min(axis=0), p.max(axis=0), cam)
    if ibl:
        env = synthetic_envmap()
        tid = b.add_texture("synthetic_sky_2048x1024", env)
        b.add_ibl(tid, avg_illum=envmap_avg_illum(env))
    else:
        b.set_background((1.0, 1.0, 1.0))
    return b.build(), cam


def _light_grid(b, bmin, bmax, intensity, scale, step=5):
    """ManyLightCryteckSponzaScene's grid (scenedefs.cpp:987-1044): step^3 point lights, R / G / B in turn.  As written there,
    x and z restart from 0 (not from the box's minimum) on every row; y starts at the minimum."""
    sv = (np.asarray(bmax, np.float32) - np.asarray(bmin, np.float32)) / np.float32(step)
    colors = [(1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)]
    num = 0
    y = np.float32(bmin[1])
    for _ in range(step):
        z = np.float32(0.0)
        for _ in range(step):
            x = np.float32(0.0)
            for _ in range(step):
                b.add_point_light((float(x), float(y), float(z)), colors[num % 3], intensity, scale=scale)
                x = np.float32(x + sv[0])
                num += 1
            z = np.float32(z + sv[2])
        y = np.float32(y + sv[1])


def many_light_sponza(asset_dir=None, textures=True):
    """ManyLightCryteckSponzaScene (scenedefs.cpp:987-1056) restated on the sponza_lod stand-in: the 5 x 5 x 5 grid of point lights
    over the scene's bounding box (R / G / B in turn, intensity 500) plus one white light in front of the camera -- 126 lights.
    The reference's scene is in centimetres and scales its lights by 100; sponza_lod is in metres (its camera sits 1 unit above the
    floor), so the same irradiance needs scale = 100 / 100^2 = 0.01.  Background: black (no IBL: the lights are the scene's light)."""
    def add(b, bmin, bmax, cam):
        _light_grid(b, bmin, bmax, 500.0, 0.01)
        b.add_point_light(tuple(float(c) for c in cam["at"]), (1.0, 1.0, 1.0), 500.0, scale=0.01)
    fs, cam = sponza_lod(asset_dir, ibl=False, textures=textures, add_lights=add)
    return fs, cam


def many_light_cornell(n=8, asset_dir=None):
    """A small many-light test scene (not a reference scene): the Cornell box with white Lambert surfaces and n coloured point
    lights spread over the ceiling (no area light), black background.  White walls because ReSTIR's pixel colour carries the
    albedo TEXTURE and not the base colour (docs/RESTIR.md), so that direct light agrees with the path tracer's."""
    asset_dir = asset_dir or os.path.join(ASSETS, "cornellbox")
    b = SceneBuilder()

    def create_mtrl(name, mtype, clr, albedo, nml):
        return b.add_material(name, L.MTRL_DIFFUSE, (1.0, 1.0, 1.0))

    objs = b.load_obj(os.path.join(asset_dir, "orig.obj"), create_mtrl=create_mtrl, separate_objs=True, normal_on_the_fly=True)
    for o in objs:
        if b.objects[o]["name"] != "light":
            b.create_instance(o)
    rng = np.random.default_rng(7)
    colors = [(1.0, 0.3, 0.3), (0.3, 1.0, 0.3), (0.3, 0.3, 1.0), (1.0, 1.0, 0.6)]
    for i in range(n):
        x, z = rng.uniform(-0.8, 0.8), rng.uniform(-0.8, 0.8)
        b.add_point_light((float(x), 1.2 + 0.3 * float(rng.uniform()), float(z)), colors[i % 4], 4.0 * 8.0 / max(n, 1))
    b.set_background((0.0, 0.0, 0.0))
    cam = dict(pos=(0.0, 1.0, 3.0), at=(0.0, 1.0, 0.0), vfov=45.0)
    return b.build(), cam


def cornell_box_variant(lights="area", move_boxes=True, asset_dir=None, extra_materials=False):
    """Parity-test variant of the Cornell box (not a reference scene): the two boxes are instanced with
    non-identity matrices (translation / rotation about y, so the W2L ray transform, the L2W hit transform
    and the instance area ratio are exercised) and the light set is selectable:
      "area"  the reference's polygon light            "point" / "spot" / "directional"  punctual lights
      "mixed" area + point + spot + directional (uniform light pick among four)
      "sphere" a sphere area light (AreaLight over a sphere object; the sphere itself is never hit by rays)
    """
    asset_dir = asset_dir or os.path.join(ASSETS, "cornellbox")
    b = SceneBuilder()
    emit = b.add_material("light", L.MTRL_EMISSIVE, (1.0, 1.0, 1.0))

    def create_mtrl(name, mtype, clr, albedo, nml):
        if name == "shortBox":
            return b.add_material(name, L.MTRL_DISNEY, (0.7, 0.6, 0.5), roughness=0.35, metallic=0.3,
                                  specular=0.6, clearcoat=0.4, clearcoatGloss=0.7, sheen=0.3)
        if name == "floor":
            return b.add_material(name, L.MTRL_GGX, (0.7, 0.6, 0.5), roughness=0.1, ior=0.01)
        if extra_materials is True and name == "tallBox":       # glass (refraction.cpp), like the reference's glass spheres
            return b.add_material(name, L.MTRL_REFRACTION, (0.9, 0.9, 0.9), ior=1.5)
        if extra_materials and name == "leftWall":
            return b.add_material(name, L.MTRL_OREN_NAYAR, clr, roughness=0.6)
        if extra_materials == "rough" and name == "tallBox":     # frosted glass (microfacet_refraction.cpp)
            return b.add_material(name, L.MTRL_MICROFACET_REFRACTION, (0.9, 0.9, 0.9), ior=1.5, roughness=0.2)
        if extra_materials == "rough" and name == "rightWall":
            return b.add_material(name, L.MTRL_VELVET, clr, roughness=0.4)
        if extra_materials == "carpaint" and name == "shortBox":   # clearcoat over flakes over diffuse (car_paint.cpp)
            return b.add_carpaint_material(name, (1.0, 1.0, 1.0))
        if extra_materials == "carpaint" and name == "backWall":
            return b.add_carpaint_material(name, (0.9, 0.9, 0.9), diffuse_color=(0.1, 0.3, 0.8), flakes_color=(0.9, 0.9, 1.0),
                                           flake_size=0.4, clearcoat_ior=1.6, flake_scale=60.0)
        if extra_materials == "retro" and name == "rightWall":   # prismatic-sheet retroreflector (retroreflective.cpp)
            return b.add_material(name, L.MTRL_RETROREFLECTIVE, clr, roughness=0.3, ior=1.5)
        if extra_materials == "retro" and name == "tallBox":
            return b.add_material(name, L.MTRL_RETROREFLECTIVE, (0.9, 0.9, 0.9), roughness=0.1, ior=1.33)
        if extra_materials and name == "backWall":
            return b.add_material(name, L.MTRL_BECKMAN, (0.7, 0.7, 0.7), roughness=0.25, ior=0.2)
        return b.add_material(name, mtype, clr)

    objs = b.load_obj(os.path.join(asset_dir, "orig.obj"), create_mtrl=create_mtrl,
                      separate_objs=True, normal_on_the_fly=True)
    names = [b.objects[o]["name"] for o in objs]

    def rot_y_trans(deg, t):
        c, s_ = np.cos(np.radians(deg)), np.sin(np.radians(deg))
        return np.array([[c, 0, s_, t[0]], [0, 1, 0, t[1]], [-s_, 0, c, t[2]], [0, 0, 0, 1]], np.float32)

    inst = {}
    for o, n in zip(objs, names):
        if n == "light" and lights not in ("area", "mixed"):
            continue        # an emissive object without a registered light has light_id = -1 (the reference would index lights[-1])
        M = None
        if move_boxes and n == "tallBox":
            M = rot_y_trans(17.0, (0.15, 0.0, 0.1))
        if move_boxes and n == "shortBox":
            M = rot_y_trans(-23.0, (-0.2, 0.25, 0.05))
        inst[n] = b.create_instance(o, M)
    if lights in ("area", "mixed"):
        b.add_area_light(inst["light"], (1.0, 1.0, 1.0), 200.0)
    if lights == "sphere":
        sm = b.add_material("sphere_emit", L.MTRL_EMISSIVE, (1.0, 0.9, 0.8))
        sp = b.add_sphere((0.1, 1.55, 0.2), 0.18, sm)
        b.add_area_light(sp, (1.0, 0.9, 0.8), 30.0)
    if lights in ("point", "mixed"):
        b.add_point_light((0.3, 1.6, 0.4), (1.0, 0.9, 0.8), 40.0)
    if lights in ("spot", "mixed"):
        l = np.zeros((), L.LIGHT_PARAM)
        l["type"] = L.LIGHT_SPOT
        l["attrib"] = L.LATTR_SINGULAR
        l["pos"] = (-0.5, 1.8, 0.6, 1.0)
        d = np.array([0.3, -1.0, -0.4], np.float32)
        d /= np.linalg.norm(d)
        l["dir"] = (d[0], d[1], d[2], 0.0)
        l["light_color"] = (0.8, 0.9, 1.0)
        l["innerAngle"], l["outerAngle"] = np.radians(25.0), np.radians(60.0)
        l["scale"], l["intensity"] = 1.0, 60.0
        l["arealight_objid"], l["envmapidx"] = -1, -1
        b.lights.append(l)
    if lights in ("directional", "mixed"):
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
    b.set_background((0.02, 0.03, 0.05))
    cam = dict(pos=(0.0, 1.0, 3.0), at=(0.0, 1.0, 0.0), vfov=45.0)
    return b.build(), cam


# ---------------------------------------------------------------------------------------------------
# Procedural stand-in for BASELINE config 4 (Crytek Sponza: sponza.obj/.sbvh are missing blobs)
# ---------------------------------------------------------------------------------------------------
def _grid_mesh(fn, nu, nv, uv_scale=(1.0, 1.0), flip=False):
    """Tessellated parametric surface: fn(u, v) -> xyz for u, v in [0,1] (arrays).  Smooth vertex normals
    from central differences; two triangles per cell."""
    u = np.linspace(0.0, 1.0, nu + 1)
    v = np.linspace(0.0, 1.0, nv + 1)
    U, V = np.meshgrid(u, v, indexing="ij")
    P = fn(U, V).astype(np.float64)
    e = 1e-4
    du = fn(np.clip(U + e, 0, 1), V) - fn(np.clip(U - e, 0, 1), V)
    dv = fn(U, np.clip(V + e, 0, 1)) - fn(U, np.clip(V - e, 0, 1))
    N = np.cross(du.reshape(-1, 3), dv.reshape(-1, 3))
    N /= np.maximum(np.linalg.norm(N, axis=1, keepdims=True), 1e-20)
    if flip:
        N = -N
    idx = np.arange((nu + 1) * (nv + 1)).reshape(nu + 1, nv + 1)
    a, b_, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    tri = np.concatenate([np.stack([a, b_, c], 1), np.stack([a, c, d], 1)]) if not flip else \
        np.concatenate([np.stack([a, c, b_], 1), np.stack([a, d, c], 1)])
    uv = np.stack([U.ravel() * uv_scale[0], V.ravel() * uv_scale[1]], 1)
    return P.reshape(-1, 3).astype(np.float32), N.astype(np.float32), uv.astype(np.float32), tri


def _icosphere(level):
    t = (1.0 + 5 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
         (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10),
         (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(level):
        cache, nf = {}, []

        def mid(i, j):
            k = (min(i, j), max(i, j))
            if k not in cache:
                m = v[i] + v[j]
                v.append(m / np.linalg.norm(m))
                cache[k] = len(v) - 1
            return cache[k]
        for (a, b_, c) in f:
            ab, bc, ca = mid(a, b_), mid(b_, c), mid(c, a)
            nf += [(a, ab, ca), (b_, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.asarray(v, np.float64), np.asarray(f, np.int64)


def atrium(asset_dir=None, mtype=L.MTRL_DISNEY, detail=1.0, bvh_options=None):
    """Procedural colonnaded hall, ~250 k unique triangles (+ 6 instances of a 20 k-triangle statue), Disney
    materials with the Sponza albedo / normal-map textures, IBL + one polygon area light.  Stand-in for
    BASELINE config 4 "Crytek Sponza 4K 8spp 8-bounce Disney + textures" (≈262 k triangles), whose
    geometry blob is absent; deterministic (no RNG).  `detail` scales the tessellation."""
    asset_dir = asset_dir or os.path.join(ASSETS, "sponza")
    b = SceneBuilder()
    cam = dict(pos=(-7.0, 1.7, 0.6), at=(0.0, 1.5, 0.0), vfov=45.0)
    # the trees built here: children nearer the viewer are threaded first
    b.bvh_options = dict(order_point=cam["pos"]) if bvh_options is None else bvh_options

    def tex(name):
        return b.load_image(os.path.join(asset_dir, name))

    def mtrl(name, clr, alb, nm, **kw):
        if mtype == L.MTRL_DISNEY:
            std = dict(roughness=0.5, metallic=0.0, specular=0.5, clearcoat=0.0, clearcoatGloss=0.5, sheen=0.0)
            std.update(kw)
            return b.add_material(name, L.MTRL_DISNEY, clr, albedo_map=tex(alb) if alb else -1,
                                  normal_map=tex(nm) if nm else -1, **std)
        return b.add_material(name, mtype, clr, albedo_map=tex(alb) if alb else -1, normal_map=tex(nm) if nm else -1,
                              roughness=kw.get("roughness", 0.3), ior=0.01)

    m_floor = mtrl("floor", (0.8, 0.8, 0.8), "KAMEN.JPG", "KAMEN-nml.png", roughness=0.25, specular=0.7, clearcoat=0.3)
    m_wall = mtrl("wall", (0.8, 0.8, 0.8), "01_STUB.JPG", "01_STUB-nml.png", roughness=0.7)
    m_col = mtrl("column", (0.8, 0.8, 0.8), "sp_luk.JPG", "sp_luk-nml.png", roughness=0.55, sheen=0.2)
    m_gold = mtrl("statue", (0.9, 0.7, 0.3), None, None, roughness=0.3, metallic=0.9, specular=0.8)
    m_emit = b.add_material("lamp", L.MTRL_EMISSIVE, (1.0, 0.95, 0.9))

    def n(x):
        return max(2, int(round(x * detail)))

    X, Z, H = 8.0, 4.0, 6.0
    # floor: gentle relief
    P, N, UV, T = _grid_mesh(lambda u, v: np.stack([(2 * u - 1) * X, 0.02 * np.sin(37.0 * u) * np.cos(23.0 * v)
                                                    + 0.01 * np.sin(211.0 * u + 89.0 * v), (1 - 2 * v) * Z], -1),
                             n(320), n(160), uv_scale=(8.0, 4.0))
    hall = b.add_mesh("hall", P, T, m_floor, normals=N, uvs=UV, need_normal=False)
    # walls with brick-like relief; inward-facing
    def wall(axis, sign):
        def fn(u, v):
            relief = 0.03 * np.sin(60.0 * u) * np.sin(40.0 * v) + 0.015 * np.sin(170.0 * u + 130.0 * v)
            if axis == "z":
                return np.stack([(2 * u - 1) * X * sign, v * H, np.full_like(u, sign * Z) - sign * relief], -1)
            return np.stack([np.full_like(u, sign * X) - sign * relief, v * H, (1 - 2 * u) * Z * sign], -1)
        return _grid_mesh(fn, n(160), n(64), uv_scale=(6.0, 3.0))
    for axis, sign in (("z", 1.0), ("z", -1.0), ("x", 1.0), ("x", -1.0)):
        P, N, UV, T = wall(axis, sign)
        b.add_mesh("wall", P, T, m_wall, normals=N, uvs=UV, need_normal=False, into=hall)
    # fluted columns
    for side in (-1.0, 1.0):
        for k in range(6):
            cx, cz = -6.25 + 2.5 * k, side * 2.3

            def col(u, v, cx=cx, cz=cz):
                ang = 2 * np.pi * u
                r = 0.28 + 0.02 * np.cos(16 * ang) + 0.06 * np.exp(-40.0 * v) + 0.06 * np.exp(-40.0 * (1 - v))
                return np.stack([cx + r * np.cos(ang), v * 5.0, cz - r * np.sin(ang)], -1)
            P, N, UV, T = _grid_mesh(col, n(48), n(40), uv_scale=(2.0, 5.0))
            b.add_mesh("column", P, T, m_col, normals=N, uvs=UV, need_normal=False, into=hall)
    # lamp: one quad under the open roof
    lamp_p = np.array([[-1.0, 5.6, -0.6], [1.0, 5.6, -0.6], [1.0, 5.6, 0.6], [-1.0, 5.6, 0.6]], np.float32)
    lamp = b.add_mesh("lamp", lamp_p, [[0, 1, 2], [0, 2, 3]], m_emit)
    # statue: displaced icosphere, instanced
    V, F = _icosphere(5 if detail >= 1.0 else 3)
    disp = 1.0 + 0.12 * np.sin(7.0 * V[:, 0]) * np.sin(9.0 * V[:, 1]) * np.sin(5.0 * V[:, 2]) + 0.05 * np.sin(23.0 * V[:, 1])
    SP = (V * disp[:, None]).astype(np.float32)
    statue = b.add_mesh("statue", SP, F, m_gold, need_normal=True)

    def trs(scale, deg, t):
        c, s_ = np.cos(np.radians(deg)), np.sin(np.radians(deg))
        return np.array([[c * scale, 0, s_ * scale, t[0]], [0, scale, 0, t[1]], [-s_ * scale, 0, c * scale, t[2]],
                         [0, 0, 0, 1]], np.float32)

    b.create_instance(hall)
    li = b.create_instance(lamp)
    b.add_area_light(li, (1.0, 0.95, 0.9), 60.0)
    for k in range(6):
        b.create_instance(statue, trs(0.45 + 0.05 * (k % 3), 30.0 * k, (-5.0 + 2.0 * k, 0.62 + 0.05 * (k % 3), (-1) ** k * 0.9)))
    env = synthetic_envmap()
    tid = b.add_texture("synthetic_sky_2048x1024", env)
    b.add_ibl(tid, avg_illum=envmap_avg_illum(env))
    return b.build(), cam


def blob_mesh(t, nu=48, nv=24, centre=(0.33, 1.05, 0.35), radius=0.3):
    """A UV sphere whose radius is modulated by two travelling waves of phase t: the stand-in for the reference's
    skinned character (asset/converted_unitychan, absent from the snapshot) in the deformation-renderer sequence.
    Returns (positions [V,3], normals [V,3], indices [2 nu nv, 3])."""
    f = np.float32
    th = (np.arange(nv + 1, dtype=f) / f(nv)) * f(np.pi)
    ph = (np.arange(nu, dtype=f) / f(nu)) * f(2 * np.pi)
    TH, PH = np.meshgrid(th, ph, indexing="ij")
    r = f(radius) * (f(1) + f(0.25) * np.sin(f(3) * PH + f(t)) * np.sin(f(2) * TH) + f(0.15) * np.sin(f(5) * TH - f(2 * t)))
    d = np.stack([np.sin(TH) * np.cos(PH), np.cos(TH), np.sin(TH) * np.sin(PH)], axis=-1).astype(f)
    pos = (np.asarray(centre, f)[None, None, :] + r[..., None] * d).reshape(-1, 3).astype(f)
    nml = d.reshape(-1, 3)
    idx = []
    for i in range(nv):
        for j in range(nu):
            a, b = i * nu + j, i * nu + (j + 1) % nu
            c, e = a + nu, b + nu
            idx.append((a, c, b)); idx.append((b, c, e))
    return pos, nml, np.asarray(idx, np.int64)


def deformable_room(t=0.0, asset_dir=None, **blob):
    """The Cornell box with a deforming mesh in it (the reference's deformation renderer puts a skinned model in a
    room: src/deformation_renderer/main.cpp:262-340, scenedefs.cpp DeformScene).  Returns (builder, blob object id,
    camera): call builder.build() for the scene at phase t, builder.set_mesh_vertices(...) + build() for the next."""
    asset_dir = asset_dir or os.path.join(ASSETS, "cornellbox")
    b = SceneBuilder()
    emit = b.add_material("light", L.MTRL_EMISSIVE, (1.0, 1.0, 1.0))
    objs = b.load_obj(os.path.join(asset_dir, "orig.obj"), create_mtrl=lambda name, mt, clr, a, n: b.add_material(name, mt, clr),
                      separate_objs=True, normal_on_the_fly=True)
    light = b.create_instance(objs[0])
    b.add_area_light(light, b.materials[emit][1]["baseColor"][:3], 200.0)
    for o in objs[1:]:
        b.create_instance(o)
    skin = b.add_material("skin", L.MTRL_GGX, (0.8, 0.45, 0.3), roughness=0.35, ior=1.4)
    pos, nml, idx = blob_mesh(t, **blob)
    oid = b.add_mesh("blob", pos, idx, skin, normals=nml, deformable=True)
    b.create_instance(oid)
    b.set_background((0.0, 0.0, 0.0))
    cam = dict(pos=(0.0, 1.0, 3.0), at=(0.0, 1.0, 0.0), vfov=45.0)
    return b, oid, cam


def _skin_chain(n_bones, base=(0.33, 0.12, 0.3), height=1.5):
    """Joint j of the bone chain in the bind pose: `base` + j * (0, height / n_bones, 0)."""
    return np.asarray(base, np.float64), float(height) / n_bones


def skinned_pose(t, n_bones):
    """The mat4 palette of skinned_room's bone chain at phase t: palette[j] = (joint j's pose) * (joint j's bind pose)^-1, each
    joint bending a little further than its parent around z and x.  skinned_pose(0, n) is not the identity (the chain has a
    phase per joint); an all-identity palette returns the rest pose.  float32 [n_bones, 4, 4], row-major, applied as M * p."""
    base, seg = _skin_chain(n_bones)

    def trans(v):
        m = np.eye(4); m[:3, 3] = v
        return m

    def rot(az, ax):
        cz, sz, cx, sx = np.cos(az), np.sin(az), np.cos(ax), np.sin(ax)
        rz = np.array([[cz, -sz, 0, 0], [sz, cz, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]])
        rx = np.array([[1, 0, 0, 0], [0, cx, -sx, 0], [0, sx, cx, 0], [0, 0, 0, 1.0]])
        return rz @ rx
    out = np.zeros((n_bones, 4, 4), np.float32)
    world = trans(base)
    for j in range(n_bones):
        amp = 0.7 / n_bones
        world = world @ (trans((0.0, seg, 0.0)) if j else np.eye(4)) @ rot(amp * np.sin(t + 0.6 * j), 0.6 * amp * np.cos(0.7 * t + 0.4 * j))
        out[j] = (world @ trans(-(base + np.array([0.0, j * seg, 0.0])))).astype(np.float32)
    return out


def skinned_room(nu=48, nv=24, n_bones=8, asset_dir=None, radius=0.13):
    """The Cornell box with a skinned tube in it: the stand-in for the reference's skinned character (asset/converted_unitychan, a
    blob that is absent from the snapshot) in the deformation-renderer sequence, with what a character has -- a bone chain, a
    weight falloff over two to four bones, and rings of vertices bound to a single bone.
    2 nu nv triangles, built with add_mesh(deformable=True).  Returns (builder, tube object id, camera, vertices): `vertices`
    is the aten::SkinningVertex array (layout.SKINNING_VERTEX) in the order of the scene's vertices of the tube -- the builder
    stores three vertices per triangle -- for atn_skin_create; skinned_pose(t, n_bones) is its palette."""
    asset_dir = asset_dir or os.path.join(ASSETS, "cornellbox")
    b = SceneBuilder()
    emit = b.add_material("light", L.MTRL_EMISSIVE, (1.0, 1.0, 1.0))
    objs = b.load_obj(os.path.join(asset_dir, "orig.obj"), create_mtrl=lambda name, mt, clr, a, n: b.add_material(name, mt, clr),
                      separate_objs=True, normal_on_the_fly=True)
    light = b.create_instance(objs[0])
    b.add_area_light(light, b.materials[emit][1]["baseColor"][:3], 200.0)
    for o in objs[1:]:
        b.create_instance(o)
    mtrl = b.add_material("skin", L.MTRL_GGX, (0.8, 0.45, 0.3), roughness=0.35, ior=1.4)
    base, seg = _skin_chain(n_bones)
    f = np.float32
    ph = (np.arange(nu, dtype=np.float64) / nu) * 2 * np.pi
    hv = np.arange(nv + 1, dtype=np.float64) / nv
    HV, PH = np.meshgrid(hv, ph, indexing="ij")
    d = np.stack([np.cos(PH), np.zeros_like(PH), np.sin(PH)], axis=-1)
    pos = (base[None, None, :] + radius * d + np.stack([np.zeros_like(HV), HV * seg * n_bones, np.zeros_like(HV)], -1)).reshape(-1, 3).astype(f)
    nml = d.reshape(-1, 3).astype(f)
    uv = np.stack([PH / (2 * np.pi), HV], -1).reshape(-1, 2).astype(f)
    idx = []
    for i in range(nv):
        for j in range(nu):
            a, c = i * nu + j, i * nu + (j + 1) % nu
            idx.append((a, a + nu, c)); idx.append((c, a + nu, c + nu))
    idx = np.asarray(idx, np.int64)
    # weights: a tent of half-width 2 bones around the vertex (two to four bones); every fourth ring of vertices follows its bone alone
    s = np.clip(HV.reshape(-1) * n_bones, 0.0, n_bones - 1e-6)
    b0 = np.floor(s).astype(np.int64)
    cand = b0[:, None] + np.array([-1, 0, 1, 2])[None, :]
    w = np.maximum(0.0, 1.0 - np.abs(s[:, None] - (cand + 0.5)) / 2.0)
    w[(cand < 0) | (cand >= n_bones)] = 0.0
    single = (np.arange(nv + 1)[:, None] % 4 == 2).repeat(nu, 1).reshape(-1)
    w[single] = np.array([0.0, 1.0, 0.0, 0.0])
    w /= w.sum(1, keepdims=True)
    cand = np.clip(cand, 0, n_bones - 1)        # (a weight of 0 still names a matrix: all four are read)
    sv = np.zeros(len(pos), L.SKINNING_VERTEX)
    sv["position"][:, :3] = pos; sv["position"][:, 3] = 1.0
    sv["normal"] = nml; sv["clr"] = 255; sv["uv"] = uv
    sv["blend_index"] = cand.astype(f); sv["blend_weight"] = w.astype(f)
    oid = b.add_mesh("tube", pos, idx, mtrl, normals=nml, uvs=uv, deformable=True)
    b.create_instance(oid)
    b.set_background((0.0, 0.0, 0.0))
    cam = dict(pos=(0.0, 1.0, 3.0), at=(0.0, 1.0, 0.0), vfov=45.0)
    return b, oid, cam, np.ascontiguousarray(sv[idx.reshape(-1)])


MOVING_QUAD = dict(centre=(-0.2, 1.55, -0.6), half=(0.3, 0.25))


def moving_quad_room(offset=0.0, asset_dir=None, second_offset=None):
    """The Cornell box with a camera-facing quad in front of its back wall, as a rigid instance translated along camera-right (+x
    for this camera) by `offset`: the moved-instance case of the geometry motion vectors (docs/MOTION.md).  The quad's material is
    its own -- SVGF's mesh-id test compares the material id, so history from the wall behind it is rejected.  Every offset gives the
    same bottom-level lists: renderer.updateBVH(moving_quad_room(x)[0]) moves the instance.  The quad spans
    MOVING_QUAD["centre"] +- MOVING_QUAD["half"] in x and y (before the translation), above the tall box, in the plane z = centre z.
    second_offset: a second instance of the same quad, translated by that much and 0.55 downwards (one more object and matrix pair
    over the same lists, appended behind everything else: the first instance keeps its ids).
    Returns (FlatScene, camera, dict(instance=object id of the quad's instance, mtx_id=its L2W matrix, mtrl=its material id))."""
    asset_dir = asset_dir or os.path.join(ASSETS, "cornellbox")
    b = SceneBuilder()
    emit = b.add_material("light", L.MTRL_EMISSIVE, (1.0, 1.0, 1.0))
    objs = b.load_obj(os.path.join(asset_dir, "orig.obj"), create_mtrl=lambda name, mt, clr, a, n: b.add_material(name, mt, clr),
                      separate_objs=True, normal_on_the_fly=True)
    light = b.create_instance(objs[0])
    b.add_area_light(light, b.materials[emit][1]["baseColor"][:3], 200.0)
    for o in objs[1:]:
        b.create_instance(o)
    mtrl = b.add_material("quad", L.MTRL_DIFFUSE, (0.2, 0.6, 0.8))
    (cx, cy, cz), (hx, hy) = MOVING_QUAD["centre"], MOVING_QUAD["half"]
    pos = np.array([[cx - hx, cy - hy, cz], [cx + hx, cy - hy, cz], [cx + hx, cy + hy, cz], [cx - hx, cy + hy, cz]], np.float32)
    nml = np.tile(np.array([0.0, 0.0, 1.0], np.float32), (4, 1))
    oid = b.add_mesh("quad", pos, np.array([[0, 1, 2], [0, 2, 3]], np.int64), mtrl, normals=nml)
    M = np.eye(4, dtype=np.float32)
    M[0, 3] = offset
    inst = b.create_instance(oid, M)
    if second_offset is not None:
        M2 = np.eye(4, dtype=np.float32)
        M2[0, 3], M2[1, 3] = second_offset, -0.55
        b.create_instance(oid, M2)
    b.set_background((0.0, 0.0, 0.0))
    cam = dict(pos=(0.0, 1.0, 3.0), at=(0.0, 1.0, 0.0), vfov=45.0)
    return b.build(), cam, dict(instance=inst, mtx_id=b.objects[inst]["mtx_id"], mtrl=mtrl)


def toon_ramp(steps=(0.15, 0.45, 0.8, 1.0), width=64, tint=(1.0, 1.0, 1.0)):
    """A 1-D remap texture (ToonParameter::remap_texture): `width` texels in `len(steps)` flat bands."""
    t = np.ones((1, width, 4), np.float32)
    for x in range(width):
        b = steps[min(x * len(steps) // width, len(steps) - 1)]
        t[0, x, :3] = [b * c for c in tint]
    return t


def toon_room(asset_dir=None, target="point", screen_shadow=None, alpha_blocker=False, stylized_shadow=(), without=()):
    """The Cornell box with NPR materials (material/toon.cpp): the tall box is a Toon material of diffuse type, the short
    box a StylizedBrdf of specular type with a stylised highlight and a rim light, the floor a Toon material of specular type;
    all aim at ONE NPR target light (context::AddNprTargetLight) -- a point light, or the room's area light -- and the
    area light still lights the rest of the room.  `screen_shadow` [h, w]: the screen-space shadow texture of the
    stylized-shadow feature (enabled on the tall box when given).  `stylized_shadow`: names of toon materials ("tallBox", "floor")
    that enable the feature whether or not a texture is given; `without`: material names whose objects are left out of the room."""
    asset_dir = asset_dir or os.path.join(ASSETS, "cornellbox")
    b = SceneBuilder()
    shadow_term = dict(shadow_enable=1, shadow_threshold=0.9, shadow_offset=0.05, shadow_scale=1.0)
    left_out = []
    emit = b.add_material("light", L.MTRL_EMISSIVE, (1.0, 1.0, 1.0))
    ramp = b.add_texture("ramp4", toon_ramp())
    ramp_warm = b.add_texture("ramp3warm", toon_ramp((0.2, 0.6, 1.0), tint=(1.0, 0.85, 0.6)))

    def create_mtrl(name, mtype, clr, albedo, nml):
        mid = create_mtrl_named(name, mtype, clr)
        if name in without:
            left_out.append(mid)
        return mid

    def create_mtrl_named(name, mtype, clr):
        if name == "tallBox":
            extra = shadow_term if (screen_shadow is not None or name in stylized_shadow) else {}
            return b.add_toon_material(name, (0.9, 0.5, 0.4), target_light_idx=0, remap_texture=ramp, **extra)
        if name == "shortBox":
            return b.add_toon_material(name, (0.4, 0.6, 0.9), stylized=True, toon_type=L.MTRL_SPECULAR, target_light_idx=0,
                                       remap_texture=ramp_warm, roughness=0.3, ior=1.5, stylized_y_min=0.05, stylized_y_max=0.6,
                                       translation_dt=0.1, translation_db=-0.05, scale_t=0.2, scale_b=0.1, split_t=0.05, split_b=0.02,
                                       square_sharp=0.7, square_magnitude=0.3,
                                       rim_enable=1, rim_width=0.4, rim_softness=0.3, rim_color=(0.3, 0.5, 1.0), rim_spread=1.0)
        if name == "floor":
            return b.add_toon_material(name, (0.7, 0.7, 0.6), toon_type=L.MTRL_SPECULAR, target_light_idx=0, remap_texture=-1,
                                       roughness=0.4, ior=1.4, will_receive_shadow=1, **(shadow_term if name in stylized_shadow else {}))
        return b.add_material(name, mtype, clr)

    objs = b.load_obj(os.path.join(asset_dir, "orig.obj"), create_mtrl=create_mtrl, separate_objs=True, normal_on_the_fly=True)
    light = b.create_instance(objs[0])
    lid = b.add_area_light(light, b.materials[emit][1]["baseColor"][:3], 200.0)
    for o in objs[1:]:
        if not (left_out and all(m["mtrl"] in left_out for m in b.objects[o]["meshes"])):
            b.create_instance(o)
    if alpha_blocker:
        glass = b.add_material("pane", L.MTRL_DIFFUSE, (0.9, 0.9, 0.9, 0.5))
        b.config.enable_alpha_blending = 1
        q = np.array([[-0.6, 1.5, -0.4], [0.6, 1.5, -0.4], [0.6, 1.5, 0.6], [-0.6, 1.5, 0.6]], np.float32)
        b.create_instance(b.add_mesh("pane", q, [[0, 1, 2], [0, 2, 3]], glass))
    if target == "point":
        l = np.zeros((), L.LIGHT_PARAM)
        l["type"] = L.LIGHT_POINT; l["attrib"] = L.LATTR_SINGULAR
        l["pos"] = [0.3, 1.7, 1.2, 1.0]; l["light_color"] = (1.0, 1.0, 1.0)
        l["innerAngle"] = l["outerAngle"] = np.pi
        l["scale"], l["intensity"] = 1.0, 4.0
        l["arealight_objid"] = -1; l["envmapidx"] = -1
        b.add_npr_target_light(l)
    else:
        b.add_npr_target_light(b.lights[lid])
    if screen_shadow is not None:
        sst = np.zeros(screen_shadow.shape + (4,), np.float32)
        sst[..., 0] = screen_shadow
        b.screen_space_texture = sst
    b.set_background((0.0, 0.0, 0.0))
    cam = dict(pos=(0.0, 1.0, 3.0), at=(0.0, 1.0, 0.0), vfov=45.0)
    return b.build(), cam


def with_feature_lines(scene, enabled=True, color=(0.0, 0.0, 0.0), width=1.5, albedo_threshold=0.1, normal_threshold=0.1,
                       materials=None, metric_flag=15):
    """A built scene with feature lines (PathTracing.npr_render): FeatureLineConfig in the scene rendering config and
    FeatureLineMtrlConfig = (1, metric_flag) on the materials named by index in `materials` (None = all; [] = none).  Writes the
    same bytes SceneBuilder.set_feature_line / add_material(feature_line=...) write."""
    from .builder import write_feature_line_config, write_feature_line_mtrl
    fs, cam = scene
    write_feature_line_config(fs.desc.config, enabled, color, width, albedo_threshold, normal_threshold)
    mats = fs.arrays["materials"]
    for i in range(len(mats)):
        on = materials is None or i in materials
        write_feature_line_mtrl(mats[i], 1 if on else 0, metric_flag if on else 0)
    return fs, cam


def stylized_shadow_room(asset_dir=None, target="point", alpha_blocker=False, short_box=True):
    """toon_room with the stylized shadow term (ToonParameter::stylized_shadow) enabled on the tall box AND the floor, and no
    uploaded screen-space texture: the scene of the NPR shadow pre-pass (PathTracing.set_npr_shadow(1); docs/NPR_SHADOW.md), which
    makes the texture per frame.  Toon pixels lit and in the boxes' shadows, non-toon walls, the lamp, background pixels (the camera is
    toon_room's with a wider field of view).
    `short_box=False` leaves the short box out (what its shadow on the floor is measured against)."""
    fs, cam = toon_room(asset_dir, target=target, alpha_blocker=alpha_blocker, stylized_shadow=("tallBox", "floor"),
                        without=() if short_box else ("shortBox",))
    # (a wider view than toon_room's: the background shows around the box's open front at every aspect ratio)
    return fs, dict(cam, vfov=56.0)


def stylized_shadow_sponza(asset_dir=None):
    """sponza_lod with every second material a Toon material of diffuse type that enables the stylized shadow term, aiming at a point
    NPR target light under the roof; the others keep their GGX parameters and the synthetic sky lights the scene: the benchmark scene
    of the NPR shadow pre-pass (tools/npr_shadow_bench.py)."""
    def mtrl(b, name, clr, alb, nm):
        if len(b.materials) % 2:
            return b.add_material(name, L.MTRL_GGX, clr, albedo_map=alb, normal_map=nm, roughness=0.3, ior=0.01)
        ramp = b.add_texture("ramp4", toon_ramp())
        return b.add_toon_material(name, clr, target_light_idx=0, remap_texture=ramp, albedo_map=alb, normal_map=nm,
                                   shadow_enable=1, shadow_threshold=0.9, shadow_offset=0.05, shadow_scale=1.0)

    def target_light(b, bmin, bmax, cam):
        l = np.zeros((), L.LIGHT_PARAM)
        l["type"] = L.LIGHT_POINT; l["attrib"] = L.LATTR_SINGULAR
        l["pos"] = [0.5 * (bmin[0] + bmax[0]), bmin[1] + 0.8 * (bmax[1] - bmin[1]), 0.5 * (bmin[2] + bmax[2]), 1.0]
        l["light_color"] = (1.0, 1.0, 1.0)
        l["innerAngle"] = l["outerAngle"] = np.pi
        l["scale"], l["intensity"] = 1.0, 40.0
        l["arealight_objid"] = -1; l["envmapidx"] = -1
        b.add_npr_target_light(l)

    return sponza_lod(asset_dir, mtype=mtrl, add_lights=target_light)


def npr_room(asset_dir=None, **lines):
    """toon_room (point target light, no stylized shadow) with black feature lines on every material."""
    return with_feature_lines(toon_room(asset_dir), **lines)


def npr_sponza(asset_dir=None, **lines):
    """sponza_lod with GGX materials -- glossy, so sample rays keep bouncing -- and black feature lines on every material: the NPR
    benchmark scene."""
    return with_feature_lines(sponza_lod(asset_dir), **lines)


# ---------------------------------------------------------------------------------------------------
# Homogeneous media (PathTracing.volume_render; docs/VOLUME.md), after scenedefs.cpp:1058-1250
# ---------------------------------------------------------------------------------------------------
def _box_mesh(bmin, bmax):
    """An axis-aligned box as 12 triangles wound so that the geometric normals face outwards."""
    x0, y0, z0 = bmin
    x1, y1, z1 = bmax
    p = np.array([(x0, y0, z0), (x1, y0, z0), (x1, y1, z0), (x0, y1, z0), (x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1)], np.float32)
    quads = [(0, 3, 2, 1), (4, 5, 6, 7), (0, 4, 7, 3), (1, 2, 6, 5), (0, 1, 5, 4), (3, 7, 6, 2)]      # -z +z -x +x -y +y
    tri = np.array([t for (a, b_, c, d) in quads for t in ((a, b_, c), (a, c, d))], np.int64)
    return p, tri


def _cornell_with(create_mtrl, light_intensity=20.0):
    b = SceneBuilder()
    emit = b.add_material("light", L.MTRL_EMISSIVE, (1.0, 1.0, 1.0))
    objs = b.load_obj(os.path.join(ASSETS, "cornellbox", "orig.obj"), create_mtrl=lambda *a: create_mtrl(b, *a),
                      separate_objs=True, normal_on_the_fly=True)
    light = b.create_instance(objs[0])
    b.add_area_light(light, b.materials[emit][1]["baseColor"][:3], light_intensity)
    for o in objs[1:]:
        b.create_instance(o)
    b.set_background((0.0, 0.0, 0.0))
    return b, dict(pos=(0.0, 1.0, 3.0), at=(0.0, 1.0, 0.0), vfov=45.0)


def cornell_box_medium():
    """CornellBoxHomogeneousMediumScene (scenedefs.cpp:1121-1190): orig.obj with shortBox and tallBox as homogeneous media
    (g -0.4, sigma_a 0.5, sigma_s 0.5, le red / green)."""
    def create_mtrl(b, name, mtype, clr, albedo, nml):
        if name == "shortBox":
            return b.add_medium_material(name, -0.4, 0.5, 0.5, (1.0, 0.0, 0.0))
        if name == "tallBox":
            return b.add_medium_material(name, -0.4, 0.5, 0.5, (0.0, 1.0, 0.0))
        return b.add_material(name, mtype, clr)
    b, cam = _cornell_with(create_mtrl)
    return b.build(), cam


def cornell_box_smoke(bmin=(-0.9, 0.02, -0.9), bmax=(0.9, 1.5, 0.9)):
    """CornellBoxSmokeScene (scenedefs.cpp:1058-1118) with the smoke box built here instead of box_smoke.obj: the Cornell box with a
    box of smoke (g -0.4, sigma_a 0, sigma_s 0.5, le red) around the two boxes -- surfaces inside a medium, connections that leave it."""
    b, cam = _cornell_with(lambda b, name, mtype, clr, albedo, nml: b.add_material(name, mtype, clr))
    smoke = b.add_medium_material("medium", -0.4, 0.0, 0.5, (1.0, 0.0, 0.0))
    p, tri = _box_mesh(bmin, bmax)
    b.create_instance(b.add_mesh("smoke", p, tri, smoke))
    return b.build(), cam


def cornell_box_subsurface(center=(0.0, 0.6, 0.2), radius=0.45, level=3):
    """HomogeneousMediumRefractionBunnyScene (scenedefs.cpp:1192-1250) with an icosphere standing in for the bunny (its mesh is a
    missing blob): a Refraction surface (ior 1.333) with an interior (g 0.4, sigma_a 0, sigma_s 0.9, le 0.8) in the empty Cornell box."""
    def create_mtrl(b, name, mtype, clr, albedo, nml):
        return b.add_material(name, mtype, clr)
    b = SceneBuilder()
    emit = b.add_material("light", L.MTRL_EMISSIVE, (1.0, 1.0, 1.0))
    objs = b.load_obj(os.path.join(ASSETS, "cornellbox", "orig.obj"), create_mtrl=lambda *a: create_mtrl(b, *a),
                      separate_objs=True, normal_on_the_fly=True)
    light = b.create_instance(objs[0])
    b.add_area_light(light, b.materials[emit][1]["baseColor"][:3], 20.0)
    short_box, tall_box = b.find_material("shortBox"), b.find_material("tallBox")
    for o in objs[1:]:
        mtrls = {m["mtrl"] for m in b.objects[o]["meshes"]}
        if mtrls & {short_box, tall_box}:
            continue        # the two boxes make room for the sphere
        b.create_instance(o)
    mid = b.add_material("material_0", L.MTRL_REFRACTION, (0.58, 0.58, 0.58), ior=1.333, roughness=0.011,
                         medium=dict(g=0.4, sigma_a=0.0, sigma_s=0.9, le=(0.8, 0.8, 0.8)))
    v, f = _icosphere(level)
    p = (v * radius + np.asarray(center, np.float64)).astype(np.float32)
    # face normals, as the reference loads its meshes here (ObjLoader::Load(..., true, true)): with interpolated normals a grazing
    # connection can read "leaving" off the shading normal while it geometrically enters, and step along the surface facet by facet
    b.create_instance(b.add_mesh("sphere", p, f, mid, need_normal=True))
    b.set_background((0.0, 0.0, 0.0))
    return b.build(), dict(pos=(0.0, 1.0, 3.0), at=(0.0, 1.0, 0.0), vfov=45.0)


def fog_sponza(sigma_s=0.15, g=0.2):
    """sponza_lod with a slab of thin fog across the nave, the camera outside the slab: the volume benchmark scene.  (A camera inside
    a closed medium starts with an empty medium stack, as in the reference: the medium would not be seen from inside.)"""
    def add_fog(b, bmin, bmax, cam):
        fog = b.add_medium_material("fog", g, 0.0, sigma_s, (0.0, 0.0, 0.0))
        lo = np.asarray(bmin, np.float64) + 0.02 * (np.asarray(bmax, np.float64) - np.asarray(bmin, np.float64))
        hi = np.asarray(bmax, np.float64) - 0.02 * (np.asarray(bmax, np.float64) - np.asarray(bmin, np.float64))
        # in front of the camera (it looks down -z from z = 3): the slab ends before it
        hi[2] = min(hi[2], cam["pos"][2] - 1.0)
        lo[2] = min(lo[2], hi[2] - 1.0)
        p, tri = _box_mesh(tuple(lo), tuple(hi))
        b.create_instance(b.add_mesh("fog", p, tri, fog))
    return sponza_lod(add_lights=add_fog)


def absorbing_slab(sigma=1.0, thickness=1.0, bg=(1.0, 1.0, 1.0), half=50.0):
    """One Volume box (sigma_s 0, le 0: an absorbing slab, z in [-thickness, 0], +-half wide) in front of a constant background, no
    lights: the film estimates bg * exp(-sigma * chord) (Beer-Lambert).  The camera looks down -z from z = 2."""
    b = SceneBuilder()
    m = b.add_medium_material("slab", 0.0, sigma, 0.0, (0.0, 0.0, 0.0))
    p, tri = _box_mesh((-half, -half, -thickness), (half, half, 0.0))
    b.create_instance(b.add_mesh("slab", p, tri, m))
    b.set_background(bg)
    return b.build(), dict(pos=(0.0, 0.0, 2.0), at=(0.0, 0.0, 0.0), vfov=45.0)


def ao_room(asset_dir=None, pane_height=0.25):
    """toon_room(alpha_blocker=True)'s geometry with plain diffuse materials: the AO test scene (PathTracing.ao_render).  The
    half-transparent pane (alpha 0.5) hangs `pane_height` above the floor: AO rays that start under it pass through it
    (material::isTranslucentByAlpha).  At the default height and an AO radius of 1.0 the CPU twin counts far more than 50 such rays
    at 64 x 48 (the CPU tests assert it)."""
    asset_dir = asset_dir or os.path.join(ASSETS, "cornellbox")
    b = SceneBuilder()
    emit = b.add_material("light", L.MTRL_EMISSIVE, (1.0, 1.0, 1.0))
    objs = b.load_obj(os.path.join(asset_dir, "orig.obj"), create_mtrl=lambda name, mtype, clr, albedo, nml: b.add_material(name, L.MTRL_DIFFUSE, clr),
                      separate_objs=True, normal_on_the_fly=True)
    light = b.create_instance(objs[0])
    b.add_area_light(light, b.materials[emit][1]["baseColor"][:3], 200.0)
    for o in objs[1:]:
        b.create_instance(o)
    glass = b.add_material("pane", L.MTRL_DIFFUSE, (0.9, 0.9, 0.9, 0.5))
    b.config.enable_alpha_blending = 1
    y = float(pane_height)
    q = np.array([[-0.6, y, -0.4], [0.6, y, -0.4], [0.6, y, 0.6], [-0.6, y, 0.6]], np.float32)
    b.create_instance(b.add_mesh("pane", q, [[0, 1, 2], [0, 2, 3]], glass))
    b.set_background((0.0, 0.0, 0.0))
    cam = dict(pos=(0.0, 1.0, 3.0), at=(0.0, 1.0, 0.0), vfov=45.0)
    return b.build(), cam


# ---------------------------------------------------------------------------------------------------
# Grid media (PathTracing.volume_set_grids(fs.grids); docs/VOLUME.md, "Grid media")
# ---------------------------------------------------------------------------------------------------
def cornell_box_smoke_grid(sigma_s=4.0):
    """cornell_box_smoke with a heterogeneous smoke: a cubic smoke box (side 1.5, every coordinate a binary fraction) that is exactly
    the world box of an 8 x 8 x 8 grid.  The density is a ramp in y (0.25 at the floor, 1 at the top) times a checkerboard of
    2 x 2 x 2 blocks with empty blocks between: null collisions, events and empty cells all occur.  sigma_s 4 against a largest
    density of 1 gives a majorant of 4, six expected tracking steps across the box."""
    b, cam = _cornell_with(lambda b, name, mtype, clr, albedo, nml: b.add_material(name, mtype, clr))
    z, y, x = np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij")
    density = ((0.25 + 0.75 * y / 7.0) * (((x // 2 + y // 2 + z // 2) % 2) == 0)).astype(np.float32)
    bmin, side = (-0.75, 0.0625, -0.75), 1.5
    grid = b.add_grid(density, bmin, side / 8)
    smoke = b.add_medium_material("medium", -0.4, 0.0, sigma_s, (1.0, 0.0, 0.0), grid=grid)
    p, tri = _box_mesh(bmin, tuple(c + side for c in bmin))
    b.create_instance(b.add_mesh("smoke", p, tri, smoke))
    return b.build(), cam


def smoke_grid_ragged(sigma_s=3.0):
    """The Cornell box inside a medium boundary that also holds the area light, with a 5 x 3 x 7 grid whose origin lies off the voxel
    lattice and whose box is smaller than the boundary mesh: rays miss the grid's box, cross it, or end in it at one of the two
    diffuse boxes, which stand half inside the grid; connections end at the light inside the medium but outside the grid.  A second,
    homogeneous medium straddles the front face of the boundary, so a path can enter it first and carry it at the bottom of its
    stack into the grid medium, or the other way round."""
    b, cam = _cornell_with(lambda b, name, mtype, clr, albedo, nml: b.add_material(name, mtype, clr))
    r = np.random.default_rng(7).random((7, 3, 5))
    density = np.where(r < 0.3, 0.0, r).astype(np.float32)
    grid = b.add_grid(density, (-0.53, 0.31, -0.61), 0.21)
    smoke = b.add_medium_material("smoke", 0.3, 0.0, sigma_s, (0.0, 0.0, 0.0), grid=grid)
    p, tri = _box_mesh((-0.9, 0.05, -0.9), (0.9, 1.7, 0.9))
    b.create_instance(b.add_mesh("smoke", p, tri, smoke))
    haze = b.add_medium_material("haze", -0.2, 0.1, 0.7, (0.2, 0.2, 0.6))
    p, tri = _box_mesh((-0.3, 0.9, 0.6), (0.3, 1.3, 1.2))
    b.create_instance(b.add_mesh("haze", p, tri, haze))
    return b.build(), cam


def constant_grid_slab(sigma_s=2.0, density=0.5, grid=True, box=False, majorant_scale=1.0, light=False, thickness=1.0, bg=(1.0, 1.0, 1.0), half=50.0):
    """absorbing_slab's geometry with a scattering medium (sigma_a 0): grid = True a 4 x 4 x 4 grid of constant `density` whose box
    (side 100) holds the whole slab, grid = False the homogeneous medium of sigma_s * density -- in expectation the same picture
    (docs/VOLUME.md, the acceptance rule of grid media).  box: a diffuse box stands inside the slab.  majorant_scale: the majorant
    is that many times EvalMajorant's (1: every collision is real and the two scenes draw the same paths; above 1: null collisions).
    light: a small area light stands inside the slab, facing the camera (the light inside the fog: every scatter event connects to
    it through the medium, and the connection ends inside it)."""
    b = SceneBuilder()
    if grid:
        g = b.add_grid(np.full((4, 4, 4), density, np.float32), (-half, -half, -0.75 * 2 * half), 2 * half / 4)
        m = b.add_medium_material("slab", 0.0, 0.0, sigma_s, (0.0, 0.0, 0.0), grid=g, majorant=majorant_scale * sigma_s * density)
    else:
        m = b.add_medium_material("slab", 0.0, 0.0, sigma_s * density, (0.0, 0.0, 0.0))
    p, tri = _box_mesh((-half, -half, -thickness), (half, half, 0.0))
    b.create_instance(b.add_mesh("slab", p, tri, m))
    if light:
        e = b.add_material("light", L.MTRL_EMISSIVE, (1.0, 1.0, 1.0))
        q = np.array([(-0.15, 0.35, -0.5 * thickness), (0.15, 0.35, -0.5 * thickness), (0.15, 0.65, -0.5 * thickness), (-0.15, 0.65, -0.5 * thickness)], np.float32)
        b.add_area_light(b.create_instance(b.add_mesh("light", q, [[0, 1, 2], [0, 2, 3]], e)), (1.0, 1.0, 1.0), 20.0)
    if box:
        d = b.add_material("box", L.MTRL_DIFFUSE, (0.6, 0.4, 0.2))
        p, tri = _box_mesh((-0.3, -0.3, -0.8 * thickness), (0.3, 0.3, -0.2 * thickness))
        b.create_instance(b.add_mesh("box", p, tri, d))
    b.set_background(bg)
    return b.build(), dict(pos=(0.0, 0.0, 2.0), at=(0.0, 0.0, 0.0), vfov=45.0)


def smoke_grid_sponza(sigma_s=0.6, g=0.2, n=64):
    """fog_sponza with the fog replaced by an n^3 procedural grid (a sum of three sine waves, clipped at 0, largest value 1) over the
    cube that holds the fog slab: the grid-media benchmark scene."""
    def add_smoke(b, bmin, bmax, cam):
        lo = np.asarray(bmin, np.float64) + 0.02 * (np.asarray(bmax, np.float64) - np.asarray(bmin, np.float64))
        hi = np.asarray(bmax, np.float64) - 0.02 * (np.asarray(bmax, np.float64) - np.asarray(bmin, np.float64))
        hi[2] = min(hi[2], cam["pos"][2] - 1.0)
        lo[2] = min(lo[2], hi[2] - 1.0)
        side = float((hi - lo).max())
        t = (np.arange(n) + 0.5) / n
        z, y, x = np.meshgrid(t, t, t, indexing="ij")
        d = np.sin(9.0 * x + 2.0 * y) + np.sin(7.0 * y + 3.0 * z) + np.sin(11.0 * z + 5.0 * x)
        d = np.clip(d / 3.0, 0.0, None)
        grid = b.add_grid((d / d.max()).astype(np.float32), tuple(lo), side / n)
        smoke = b.add_medium_material("smoke", g, 0.0, sigma_s, (0.0, 0.0, 0.0), grid=grid)
        p, tri = _box_mesh(tuple(lo), tuple(hi))
        b.create_instance(b.add_mesh("smoke", p, tri, smoke))
    return sponza_lod(add_lights=add_smoke)
