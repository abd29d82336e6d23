"""ctypes binding of oracle/liboracle.so.  TEST INFRASTRUCTURE ONLY: import from tests/,
__graft_entry__.smoke() and bench.py's cpu_baseline leg, never from aten_amd/."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "liboracle.so")
_lib = None


class Destination(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("maxDepth", C.c_int32),
                ("russianRouletteDepth", C.c_int32), ("sample", C.c_int32), ("frame", C.c_uint32),
                ("progressive", C.c_int32), ("nthreads", C.c_int32)]


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB):
            subprocess.check_call(["make", "-C", _HERE])
        l = C.CDLL(_LIB)
        l.orc_pixel_width_at_distance.restype = C.c_float
        l.orc_pixel_width_at_distance.argtypes = [C.c_void_p, C.c_float]
        l.orc_num_procs.restype = C.c_int
        _lib = l
    return _lib


def init_sampler(w, h, seed=0):
    out = np.zeros(w * h, np.uint32)
    lib().orc_init_sampler(C.c_void_p(out.ctypes.data), w, h, seed)
    return out


def cmj_samples(index, dimension, scramble, n):
    out = np.zeros(n, np.float32)
    lib().orc_cmj_samples(C.c_uint32(index), C.c_uint32(dimension), C.c_uint32(scramble), n, C.c_void_p(out.ctypes.data))
    return out


def cmj_samples2d(index, dimension, scramble, n):
    out = np.zeros((n, 2), np.float32)
    lib().orc_cmj_samples2d(C.c_uint32(index), C.c_uint32(dimension), C.c_uint32(scramble), n, C.c_void_p(out.ctypes.data))
    return out


def cmj_batch(index, dimension, scramble, draws=1):
    index = np.ascontiguousarray(index, np.uint32); dimension = np.ascontiguousarray(dimension, np.uint32)
    scramble = np.ascontiguousarray(scramble, np.uint32)
    out = np.zeros((len(index), draws), np.float32)
    lib().orc_cmj_batch(len(index), C.c_void_p(index.ctypes.data), C.c_void_p(dimension.ctypes.data),
                        C.c_void_p(scramble.ctypes.data), draws, C.c_void_p(out.ctypes.data))
    return out


def math_kat(kind, a, b=None, c=None):
    a = np.ascontiguousarray(a, np.float32)
    b = np.zeros_like(a) if b is None else np.ascontiguousarray(b, np.float32)
    c = np.zeros_like(a) if c is None else np.ascontiguousarray(c, np.float32)
    out = np.zeros_like(a)
    lib().orc_math_kat(kind, len(a), C.c_void_p(a.ctypes.data), C.c_void_p(b.ctypes.data), C.c_void_p(c.ctypes.data),
                       C.c_void_p(out.ctypes.data))
    return out


LIBM_KINDS = ["sinf", "cosf", "atanf", "acosf", "atan2f", "logf", "expf", "powf", "sqrtf", "div", "inversesqrt"]


def libm_probe(kind, a, b=None):
    """The oracle build's libm on arrays (kind: a name from LIBM_KINDS)."""
    a = np.ascontiguousarray(a, np.float32)
    b = np.ones_like(a) if b is None else np.ascontiguousarray(b, np.float32)
    out = np.zeros_like(a)
    lib().orc_libm_probe(LIBM_KINDS.index(kind), len(a), C.c_void_p(a.ctypes.data), C.c_void_p(b.ctypes.data), C.c_void_p(out.ctypes.data))
    return out


def create_camera(pos, at, vfov, width, height, up=(0, 1, 0), znear=0.1, zfar=10000.0):
    from aten_amd import layout as L
    cam = np.zeros((), L.CAMERA_PARAM)
    f3 = lambda v: (C.c_float * 3)(*[float(x) for x in v])
    lib().orc_create_camera(C.c_void_p(cam.ctypes.data), f3(pos), f3(at), f3(up), C.c_float(vfov),
                            C.c_float(znear), C.c_float(zfar), C.c_int32(width), C.c_int32(height))
    return cam


def pixel_width_at_distance(cam, dist):
    return float(lib().orc_pixel_width_at_distance(C.c_void_p(cam.ctypes.data), C.c_float(dist)))


def ray_offset(o, n):
    o = np.ascontiguousarray(o, np.float32); n = np.ascontiguousarray(n, np.float32)
    out = np.zeros_like(o)
    lib().orc_ray_offset(C.c_void_p(o.ctypes.data), C.c_void_p(n.ctypes.data), len(o), C.c_void_p(out.ctypes.data))
    return out


def generate_paths(cam, seeds, w, h, sample, frame):
    from aten_amd import layout as L
    rays = np.zeros(w * h, L.RAY)
    lib().orc_generate_paths(C.c_void_p(cam.ctypes.data), C.c_void_p(seeds.ctypes.data), C.c_uint32(len(seeds)),
                             w, h, sample, C.c_uint32(frame), C.c_void_p(rays.ctypes.data))
    return rays


def trace_closest(scene, rays, t_min=1e-9, t_max=np.finfo(np.float32).max):
    from aten_amd import layout as L
    out = np.zeros(len(rays), L.INTERSECTION)
    stats = np.zeros(2, np.uint64)
    lib().orc_trace_closest(scene.ref(), C.c_void_p(rays.ctypes.data), C.c_uint32(len(rays)),
                            C.c_float(t_min), C.c_float(t_max), C.c_void_p(out.ctypes.data), C.c_void_p(stats.ctypes.data))
    return out, stats


def shadow_queries(origins, directions, dist_to_light, light, stencil_always=False):
    """atn_shadow_query[n] (aten_amd.layout.SHADOW_QUERY) from arrays; light and stencil_always may be one value for all."""
    from aten_amd import layout as L
    o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
    q = np.zeros(len(o), L.SHADOW_QUERY)
    q["org"] = o
    q["dir"] = np.ascontiguousarray(directions, np.float32).reshape(len(o), 3)
    q["dist_to_light"] = np.broadcast_to(np.asarray(dist_to_light, np.float32), (len(o),))
    q["light"] = np.broadcast_to(np.asarray(light, np.int32), (len(o),))
    q["flags"] = np.broadcast_to(np.asarray(stencil_always, bool), (len(o),)).astype(np.uint32)
    return q


def shadow_visible(scene, queries, details=False):
    """HitTestToTargetLight per query (shadow_queries): uint8 [n], 1 = the light is visible.  details=True also returns the lookups
    made [n] and the last lookup's closest hit (INTERSECTION [n], objid < 0 = a miss)."""
    from aten_amd import layout as L
    q = np.ascontiguousarray(queries, L.SHADOW_QUERY)
    n_lights = int(scene.desc.n_lights) if hasattr(scene, "desc") else None
    if n_lights is not None and len(q) and (q["light"].min() < 0 or q["light"].max() >= n_lights):
        raise ValueError("light index outside the scene's lights")
    vis = np.zeros(len(q), np.uint8); lookups = np.zeros(len(q), np.int32); last = np.zeros(len(q), L.INTERSECTION)
    lib().orc_shadow_visible(scene.ref(), C.c_void_p(q.ctypes.data), C.c_uint32(len(q)), C.c_void_p(vis.ctypes.data),
                             C.c_void_p(lookups.ctypes.data), C.c_void_p(last.ctypes.data))
    return (vis, lookups, last) if details else vis


SHADE_CATEGORIES = [
    "miss_b0", "miss_deep", "miss_b1_singular", "emit_front_b0", "emit_front_deep", "emit_back", "emit_no_light", "toon_first", "toon_deep",
    "no_nee", "backface_opaque", "normal_map", "carpaint", "mtrl_neg", "stencil_always",
    "nee_point", "nee_spot", "nee_direction", "nee_area", "nee_ibl", "nee_one_light", "nee_many_lights", "nee_invalid",
    "rr_survived", "rr_lost", "rr_zero", "bsdf_rejected", "last_vertex",
]       # bit k of orc_shade_stage's category word


def shade_stage(scene, cam, seeds, records, width, height, bounce, max_depth, rr_depth, frame=0, sample=0, flavour="plain", details=False):
    """PathTracing::shade / ShadeMiss once per record (aten_amd.layout.SHADE_VERTEX) -> SHADE_RESULT [n]: what the next stages can observe.
    details=True also returns the category word [n] (bits: SHADE_CATEGORIES) and the margins float32 [n, 2]: the smallest distance of a
    branch decision from its threshold in ulps, {decisions behind a libm result, the others}."""
    from aten_amd import layout as L
    rec = np.ascontiguousarray(records, L.SHADE_VERTEX)
    call = L.shade_call(width, height, bounce, max_depth, rr_depth, frame, sample, flavour)
    out = np.zeros(len(rec), L.SHADE_RESULT); cat = np.zeros(len(rec), np.uint32); mg = np.zeros((len(rec), 2), np.float32)
    seeds = np.ascontiguousarray(seeds, np.uint32)
    rc = lib().orc_shade_stage(scene.ref(), C.c_void_p(cam.ctypes.data), C.c_void_p(seeds.ctypes.data), C.c_uint32(len(seeds)),
                               C.c_void_p(call.ctypes.data), C.c_void_p(rec.ctypes.data), C.c_uint32(len(rec)), C.c_void_p(out.ctypes.data),
                               C.c_void_p(cat.ctypes.data), C.c_void_p(mg.ctypes.data))
    if rc != 0:
        raise ValueError("orc_shade_stage: bad call or record")
    return (out, cat, mg) if details else out


def record_vertices(scene, cam, seeds, width, height, max_depth=5, rr_depth=3, frame=0, sample=0):
    """PathTracing::radiance over one sample of a frame with an observer: (records SHADE_VERTEX [m], bounce int32 [m], contrib [h, w, 4])
    -- one record per (pixel, bounce) in the order visited, the sample's Path.contrib per pixel."""
    from aten_amd import layout as L
    cap = width * height * max_depth
    rec = np.zeros(cap, L.SHADE_VERTEX); b = np.zeros(cap, np.int32); contrib = np.zeros((height, width, 4), np.float32)
    seeds = np.ascontiguousarray(seeds, np.uint32)
    d = Destination(width, height, max_depth, rr_depth, 1, frame, 1, 0)
    l = lib()
    l.orc_record_vertices.restype = C.c_int64
    m = l.orc_record_vertices(scene.ref(), C.c_void_p(cam.ctypes.data), C.c_void_p(seeds.ctypes.data), C.c_uint32(len(seeds)), C.byref(d),
                              C.c_int32(sample), C.c_void_p(rec.ctypes.data), C.c_void_p(b.ctypes.data), C.c_uint64(cap), C.c_void_p(contrib.ctypes.data))
    if m < 0:
        raise ValueError("orc_record_vertices failed")
    return rec[:m].copy(), b[:m].copy(), contrib


def evaluate_hits(scene, rays, isects):
    out = np.zeros((len(rays), 9), np.float32)
    lib().orc_evaluate_hits(scene.ref(), C.c_void_p(rays.ctypes.data), C.c_void_p(isects.ctypes.data),
                            C.c_uint32(len(rays)), C.c_void_p(out.ctypes.data))
    return out


def material_table(scene, mtrl_id, nrm, wi, index, scramble, uv):
    n = len(nrm)
    nrm = np.ascontiguousarray(nrm, np.float32); wi = np.ascontiguousarray(wi, np.float32)
    index = np.ascontiguousarray(index, np.uint32); scramble = np.ascontiguousarray(scramble, np.uint32)
    uv = np.ascontiguousarray(uv, np.float32)
    s = np.zeros((n, 7), np.float32); e = np.zeros((n, 5), np.float32)
    lib().orc_material_table(scene.ref(), C.c_int32(mtrl_id), C.c_uint32(n), C.c_void_p(nrm.ctypes.data),
                             C.c_void_p(wi.ctypes.data), C.c_void_p(index.ctypes.data), C.c_void_p(scramble.ctypes.data),
                             C.c_void_p(uv.ctypes.data), C.c_void_p(s.ctypes.data), C.c_void_p(e.ctypes.data))
    return s, e


def render_cost(scene, cam, seeds, width, height, max_depth=5, rr_depth=3, spp=1, frame=0):
    """Per-pixel {BVH node visits, triangle tests} of one frame: uint32 [h, w, 2] (and the film)."""
    film = np.zeros((height, width, 4), np.float32)
    cost = np.zeros((height, width, 2), np.uint32)
    d = Destination(width, height, max_depth, rr_depth, spp, frame, 1, 0)
    lib().orc_render_cost(scene.ref(), C.c_void_p(cam.ctypes.data), C.c_void_p(seeds.ctypes.data), C.c_uint32(len(seeds)),
                          C.byref(d), C.c_void_p(film.ctypes.data), None, C.c_void_p(cost.ctypes.data))
    return cost, film


def render(scene, cam, seeds, width, height, max_depth=5, rr_depth=3, spp=1, frame=0,
           film=None, progressive=True, nthreads=0, counters=False):
    """aten::PathTracing::render on the CPU oracle.  Returns film [h, w, 4] (row 0 = bottom)."""
    if film is None:
        film = np.zeros((height, width, 4), np.float32)
    d = Destination(width, height, max_depth, rr_depth, spp, frame, 1 if progressive else 0, nthreads)
    cnt = np.zeros(5, np.uint64)
    lib().orc_render(scene.ref(), C.c_void_p(cam.ctypes.data), C.c_void_p(seeds.ctypes.data), C.c_uint32(len(seeds)),
                     C.byref(d), C.c_void_p(film.ctypes.data), C.c_void_p(cnt.ctypes.data) if counters else None)
    return (film, cnt) if counters else film


def set_sampling_options(ibl_importance=False, tex_bilinear=False):
    """The product's optional samplers (atn_set_sampling_options) on the CPU twin.  Global: reset after use."""
    lib().orc_set_sampling_options(C.c_int32(int(ibl_importance)), C.c_int32(int(tex_bilinear)))


def sample_texture(scene, texid, uv):
    uv = np.ascontiguousarray(uv, np.float32).reshape(-1, 2)
    out = np.zeros((len(uv), 4), np.float32)
    lib().orc_sample_texture(scene.ref(), C.c_int32(texid), C.c_uint32(len(uv)), C.c_void_p(uv.ctypes.data), C.c_void_p(out.ctypes.data))
    return out


def lbvh_build(tris, bbox_min, bbox_max, vtx_pos, tri_id_offset=0, vtx_offset=0, with_keys=False):
    """idaten::LBVHBuilder::build on the CPU oracle (oracle/orc_lbvh.h): ThreadedBvhNode[2 n - 1] in the reference's
    own order (inner nodes 0 .. n-2, leaves n-1 .. 2n-2)."""
    from aten_amd import layout as L
    tris = np.ascontiguousarray(tris, L.TRIANGLE_PARAM)
    vtx_pos = np.ascontiguousarray(vtx_pos, np.float32).reshape(-1, 4)
    n = len(tris)
    out = np.zeros(2 * n - 1, L.BVH_NODE)
    codes = np.zeros(n, np.uint32); idx = np.zeros(n, np.uint32)
    f3 = lambda v: (C.c_float * 3)(*[float(x) for x in v])
    rc = lib().orc_lbvh_build(C.c_void_p(tris.ctypes.data), C.c_uint32(n), C.c_int32(tri_id_offset), f3(bbox_min), f3(bbox_max),
                              C.c_void_p(vtx_pos.ctypes.data), C.c_int32(vtx_offset), C.c_void_p(out.ctypes.data),
                              C.c_void_p(codes.ctypes.data), C.c_void_p(idx.ctypes.data))
    if rc != 0:
        raise ValueError("orc_lbvh_build: needs at least two triangles")
    return (out, codes, idx) if with_keys else out


def lbvh_hierarchy(sorted_keys):
    """buildTree (LBVHBuilder.cu:299-350) on sorted keys: (left, right, parent) of the 2 n - 1 nodes."""
    keys = np.ascontiguousarray(sorted_keys, np.uint32)
    n = len(keys)
    l = np.zeros(2 * n - 1, np.int32); r = np.zeros_like(l); p = np.zeros_like(l)
    rc = lib().orc_lbvh_hierarchy(C.c_void_p(keys.ctypes.data), C.c_uint32(n), C.c_void_p(l.ctypes.data),
                                  C.c_void_p(r.ctypes.data), C.c_void_p(p.ctypes.data))
    if rc != 0:
        raise ValueError("orc_lbvh_hierarchy: needs at least two keys")
    return l, r, p


def fill_basic_aovs(normal, p, w2c, albedo, meshid):
    """aten::FillBasicAOVs (renderer/aov.h:158-181) -> (normal_depth[4], albedo_meshid[4])."""
    f = lambda a, n: np.ascontiguousarray(a, np.float32).reshape(n)
    nd, am = np.zeros(4, np.float32), np.zeros(4, np.float32)
    a, b, c, d = f(normal, 3), f(p, 3), f(w2c, 16), f(albedo, 4)
    lib().orc_fill_basic_aovs(C.c_void_p(a.ctypes.data), C.c_void_p(b.ctypes.data), C.c_void_p(c.ctypes.data), C.c_void_p(d.ctypes.data),
                              C.c_int32(meshid), C.c_void_p(nd.ctypes.data), C.c_void_p(am.ctypes.data))
    return nd, am


def fill_basic_aovs_if_hit_miss(bg):
    """aten::FillBasicAOVsIfHitMiss (renderer/aov.h:183-198)."""
    nd, am = np.zeros(4, np.float32), np.zeros(4, np.float32)
    b = np.ascontiguousarray(bg, np.float32).reshape(4)
    lib().orc_fill_basic_aovs_if_hit_miss(C.c_void_p(b.ctypes.data), C.c_void_p(nd.ctypes.data), C.c_void_p(am.ctypes.data))
    return nd, am


class Svgf:
    """aten::SVGFRenderer on the CPU oracle (oracle/orc_svgf.h): frame-persistent AOV / moment buffers."""
    BUFFERS = dict(normal_depth=0, albedo_meshid=1, color_variance=2, moment_temporalweight=3,
                   prev_normal_depth=4, prev_albedo_meshid=5, prev_color_variance=6, prev_moment_temporalweight=7,
                   temporary_color=8, motion_depth=9, primary_position=10, atrous0=11, atrous1=12)

    def __init__(self):
        l = lib()
        l.orc_svgf_create.restype = C.c_void_p
        l.orc_svgf_get_buffer.restype = C.c_int
        self._h = C.c_void_p(l.orc_svgf_create())
        self.n = 0

    def close(self):
        if self._h:
            lib().orc_svgf_destroy(self._h)
            self._h = None

    def set_atrous_iterations(self, n):
        lib().orc_svgf_set_atrous_iterations(self._h, C.c_int32(n))

    def set_dilate_temporal_weight(self, on):
        lib().orc_svgf_set_dilate_temporal_weight(self._h, C.c_int32(int(on)))

    def set_motion_depth(self, md):
        md = np.ascontiguousarray(md, np.float32).reshape(-1, 4)
        lib().orc_svgf_set_motion_depth(self._h, C.c_void_p(md.ctypes.data), C.c_uint32(len(md)))

    def render(self, scene, cam, seeds, width, height, max_depth=5, rr_depth=3, spp=1, frame=0, compute_motion=False,
               stages=False, nthreads=0):
        """Returns the final film [h, w, 4] (and, with stages=True, the three intermediate puts [3, h, w, 4])."""
        film = np.zeros((height, width, 4), np.float32)
        st = np.zeros((3, height, width, 4), np.float32) if stages else None
        d = Destination(width, height, max_depth, rr_depth, spp, frame, 0, nthreads)
        lib().orc_svgf_render(self._h, scene.ref(), C.c_void_p(cam.ctypes.data), C.c_void_p(seeds.ctypes.data),
                              C.c_uint32(len(seeds)), C.byref(d), C.c_int32(1 if compute_motion else 0),
                              C.c_void_p(film.ctypes.data), C.c_void_p(st.ctypes.data) if stages else None)
        self.n = width * height
        self.shape = (height, width, 4)
        return (film, st) if stages else film

    def denoise(self, cam, contribs, normal_depth, albedo_meshid, primary_position, frame=0, compute_motion=False, stages=False,
                nthreads=0):
        """The filter passes alone on the caller's planes, float32 [h, w, 4] each: the twin of the product's svgf_upload of these
        four planes followed by svgf_denoise.  Returns what render returns."""
        planes = [np.ascontiguousarray(p, np.float32) for p in (contribs, normal_depth, albedo_meshid, primary_position)]
        height, width = planes[0].shape[:2]
        if any(p.shape != (height, width, 4) for p in planes):
            raise ValueError("denoise: four [h, w, 4] planes of one size")
        film = np.zeros((height, width, 4), np.float32)
        st = np.zeros((3, height, width, 4), np.float32) if stages else None
        d = Destination(width, height, 1, 1, 1, frame, 0, nthreads)
        lib().orc_svgf_denoise(self._h, C.c_void_p(cam.ctypes.data), C.byref(d), C.c_int32(1 if compute_motion else 0),
                               *[C.c_void_p(p.ctypes.data) for p in planes],
                               C.c_void_p(film.ctypes.data), C.c_void_p(st.ctypes.data) if stages else None)
        self.n = width * height
        self.shape = (height, width, 4)
        return (film, st) if stages else film

    def set_buffer(self, name, data):
        """The inverse of buffer(): overwrite one plane (BUFFERS) with float32 [h, w, 4], e.g. the history both sides start from."""
        data = np.ascontiguousarray(data, np.float32)
        height, width = data.shape[:2]
        if data.shape != (height, width, 4):
            raise ValueError("set_buffer: a [h, w, 4] plane")
        lib().orc_svgf_set_buffer.restype = C.c_int
        r = lib().orc_svgf_set_buffer(self._h, C.c_int32(self.BUFFERS[name]), C.c_int32(width), C.c_int32(height),
                                      C.c_void_p(data.ctypes.data))
        if r < 0:
            raise ValueError(name)
        self.n = width * height
        self.shape = (height, width, 4)

    def buffer(self, name):
        out = np.zeros(self.shape, np.float32)
        r = lib().orc_svgf_get_buffer(self._h, C.c_int32(self.BUFFERS[name]), C.c_void_p(out.ctypes.data))
        if r < 0:
            raise ValueError(name)
        return out
