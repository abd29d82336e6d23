"""Host-side handle over the C-ABI, named after the reference's GPU seam.

`PathTracing` exposes the calls an aten application makes on idaten::PathTracing
(src/libidaten/kernel/renderer.h:35-111, src/libidaten/kernel/pathtracing.cpp:23-153):
UpdateSceneData, updateCamera, render, reset -- every one a thin forward into libaten_amd.so.
"""
import ctypes as C

import numpy as np

from . import layout as L
from ._lib import Destination, K_NAMES, MGPU_K_NAMES, lib


class AtenAmdError(RuntimeError):
    pass


def _elem_ptr(base, first, dtype):
    """Address of element `first` of the C array at `base` (None stays None: the library reports the null pointer)."""
    return None if not base else C.c_void_p(int(base) + first * dtype.itemsize)


class PathTracing:
    def __init__(self, device=0):
        self._l = lib()
        self._ctx = C.c_void_p()
        rc = self._l.atn_create(C.byref(self._ctx), device)
        if rc != 0:
            raise AtenAmdError("atn_create failed (%d): no usable HIP device; libaten_amd has no CPU fallback" % rc)
        if self._l.atn_sizeof_scene_desc() != C.sizeof(L.SceneDesc):
            raise AtenAmdError("atn_scene_desc ABI mismatch")
        if self._l.atn_sizeof_destination() != C.sizeof(Destination):
            raise AtenAmdError("atn_destination ABI mismatch")
        self.width = self.height = 0
        self._skin_sizes = {}       # skin handle -> (vertices, triangles), for skin_buffer's output shapes

    def close(self):
        if self._ctx:
            self._l.atn_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise AtenAmdError("%s (status %d)" % (self._l.atn_last_error(self._ctx).decode(), rc))

    # ---- the reference's renderer surface
    def UpdateSceneData(self, scene):
        self._check(self._l.atn_upload_scene(self._ctx, C.cast(scene.ref(), C.c_void_p)))

    def updateBVH(self, scene, with_matrices=True):
        """idaten::Renderer::updateBVH (renderer.cpp:133-153): objects, matrices and the top layer of `scene`
        (a FlatScene whose bottom-level lists are the ones already uploaded).  with_matrices=False: the reference's
        `mtxs.empty()` form -- new objects and top layer, the uploaded matrices stay."""
        a = scene.arrays
        objs = np.ascontiguousarray(a["objects"])
        mtx = np.ascontiguousarray(a["matrices"]) if with_matrices else np.zeros((0, 4, 4), np.float32)
        top = np.ascontiguousarray(a["bvh_lists"][0])
        self._check(self._l.atn_update_tlas(self._ctx, objs.ctypes.data, len(objs), mtx.ctypes.data if len(mtx) else None,
                                            len(mtx), top.ctypes.data, len(top)))

    # ---- scene edits (docs/SCENE_EDITS.md; idaten::Renderer::updateMaterial / updateLight / UpdateTexture /
    # UpdateSceneRenderingConfig, renderer.cpp:207-252): each reads the edited data from `scene` (a SceneBuilder result, or
    # anything with its `desc`), whose counts and texture sizes are the uploaded ones.  Nothing is reset: call reset() for that.
    def updateMaterial(self, scene, first=0, n=None):
        """Materials [first, first + n) of `scene` (default: from `first` to the end) replace the uploaded ones."""
        d = scene.desc
        n = int(d.n_materials) - first if n is None else n
        self._check(self._l.atn_update_materials(self._ctx, _elem_ptr(d.materials, first, L.MATERIAL_PARAM), n, first))

    def updateLight(self, scene, npr_target=False, first=0, n=None):
        """Lights [first, first + n) of `scene`; npr_target: of its NPR target lights."""
        d = scene.desc
        base, count = (d.npr_target_lights, d.n_npr_target_lights) if npr_target else (d.lights, d.n_lights)
        n = int(count) - first if n is None else n
        self._check(self._l.atn_update_lights(self._ctx, _elem_ptr(base, first, L.LIGHT_PARAM), n, first, 1 if npr_target else 0))

    def UpdateTexture(self, scene, texid):
        """Texture `texid` of `scene` (same size as uploaded) replaces the uploaded one."""
        d = scene.desc
        if texid < 0 or texid >= int(d.n_textures):
            raise ValueError("UpdateTexture: the scene has no texture %d" % texid)
        tex = C.cast(d.textures, C.POINTER(L.TextureDesc))
        self._check(self._l.atn_update_texture(self._ctx, texid, C.byref(tex[texid])))

    def UpdateSceneRenderingConfig(self, scene):
        """The rendering config of `scene` (atn_scene_desc::config) replaces the uploaded one."""
        self._check(self._l.atn_update_rendering_config(self._ctx, C.byref(scene.desc.config)))

    # ---- dynamic geometry (the reference's deformation renderer, src/deformation_renderer/main.cpp:636-710)
    def updateGeometry(self, vtx_pos=None, vtx_nml=None, vtx_offset=0, triangles=None, tri_offset=0):
        """idaten::Renderer::updateGeometry (renderer.cpp:155-215): overwrite a vertex / triangle range of the scene."""
        from . import layout as L
        pos = None if vtx_pos is None else np.ascontiguousarray(vtx_pos, np.float32).reshape(-1, 4)
        nml = None if vtx_nml is None else np.ascontiguousarray(vtx_nml, np.float32).reshape(-1, 4)
        if pos is not None and nml is not None and len(pos) != len(nml):
            raise ValueError("updateGeometry: %d positions but %d normals (the C ABI takes ONE vertex count for both arrays)" % (len(pos), len(nml)))
        nv = len(pos) if pos is not None else (len(nml) if nml is not None else 0)
        tr = None if triangles is None else np.ascontiguousarray(triangles, L.TRIANGLE_PARAM)
        self._check(self._l.atn_update_geometry(self._ctx, pos.ctypes.data if pos is not None else None, nml.ctypes.data if nml is not None else None,
                               nv, vtx_offset, tr.ctypes.data if tr is not None else None, len(tr) if tr is not None else 0, tri_offset))

    def lbvh_rebuild_list(self, list_index, tri_offset, n_triangles, bbox_min, bbox_max):
        """idaten::LBVHBuilder::build into the renderer's node list (LBVHBuilder.cu:700-810), on the device."""
        f3 = lambda v: (C.c_float * 3)(*[float(x) for x in v])
        self._check(self._l.atn_lbvh_rebuild_list(self._ctx, list_index, tri_offset, n_triangles, f3(bbox_min), f3(bbox_max)))

    def lbvh_build(self, triangles, bbox_min, bbox_max, vtx_pos, tri_id_offset=0, vtx_offset=0, with_keys=False):
        """LBVHBuilder::build(..., threadedBvhNodes) (LBVHBuilder.cu:812-833): ThreadedBvhNode[2 n - 1] in the reference's order."""
        from . import layout as L
        tr = np.ascontiguousarray(triangles, L.TRIANGLE_PARAM)
        pos = np.ascontiguousarray(vtx_pos, np.float32).reshape(-1, 4)
        n = len(tr)
        out = np.zeros(max(2 * n - 1, 1), L.BVH_NODE)
        codes = np.zeros(max(n, 1), np.uint32); idx = np.zeros(max(n, 1), np.uint32)
        f3 = lambda v: (C.c_float * 3)(*[float(x) for x in v])
        self._check(self._l.atn_lbvh_build(self._ctx, tr.ctypes.data, n, tri_id_offset, f3(bbox_min), f3(bbox_max), pos.ctypes.data, len(pos),
                                           vtx_offset, out.ctypes.data, codes.ctypes.data, idx.ctypes.data))
        return (out, codes, idx) if with_keys else out

    # ---- skinning on the device (idaten::Skinning, src/libidaten/kernel/Skinning.cu; docs/SKINNING.md)
    def skin_create(self, vertices, vtx_offset, tri_offset, n_triangles, n_matrices):
        """Skinning::initWithTriangles + setVtxOffset: binds SkinningVertex records to a vertex / triangle range of the uploaded
        scene; returns the skin's handle."""
        v = np.ascontiguousarray(vertices, L.SKINNING_VERTEX)
        h = C.c_uint32(0)
        self._check(self._l.atn_skin_create(self._ctx, v.ctypes.data, len(v), vtx_offset, tri_offset, n_triangles, n_matrices, C.byref(h)))
        self._skin_sizes[h.value] = (len(v), n_triangles)
        return h.value

    def skin_update(self, skin, matrices):
        """Skinning::update: the mat4 palette of the next skin_compute."""
        m = np.ascontiguousarray(matrices, np.float32).reshape(-1, 4, 4)
        self._check(self._l.atn_skin_update(self._ctx, skin, m.ctypes.data, len(m)))

    def skin_compute(self, skin, is_restart=False, want_bbox=True):
        """Skinning::compute on the device, behind the frames in flight.  want_bbox: wait and return (min, max) as the reference
        does; False: return None at once, the box stays in device memory (lbvh_rebuild_list_skinned reads it there)."""
        if not want_bbox:
            self._check(self._l.atn_skin_compute(self._ctx, skin, int(bool(is_restart)), None, None))
            return None
        mn, mx = np.zeros(3, np.float32), np.zeros(3, np.float32)
        self._check(self._l.atn_skin_compute(self._ctx, skin, int(bool(is_restart)), mn.ctypes.data, mx.ctypes.data))
        return mn, mx

    def lbvh_rebuild_list_skinned(self, list_index, skin):
        """lbvh_rebuild_list over the skin's triangles, normalised by the skin's box as it lies in device memory."""
        self._check(self._l.atn_lbvh_rebuild_list_skinned(self._ctx, list_index, skin))

    # ---- the top layer rebuilt on the device (docs/TLAS.md)
    def tlas_rebuild(self, objects=None, matrices=None, force_general=False):
        """atn_tlas_rebuild: the top layer as an LBVH over the instances' world boxes, built on the device behind the frames in
        flight.  objects (layout.OBJECT_PARAM) / matrices (float32 [n, 4, 4]): as updateBVH's; None keeps the uploaded ones."""
        objs = None if objects is None else np.ascontiguousarray(objects, L.OBJECT_PARAM)
        mtx = None if matrices is None else np.ascontiguousarray(matrices, np.float32).reshape(-1, 4, 4)
        self._check(self._l.atn_tlas_rebuild(self._ctx, objs.ctypes.data if objs is not None else None, len(objs) if objs is not None else 0,
                                             mtx.ctypes.data if mtx is not None and len(mtx) else None, len(mtx) if mtx is not None else 0,
                                             1 if force_general else 0))

    def tlas_records(self):
        """For tests (waits for everything): the top layer's device records, the root first, as (records, root_link, top_base) --
        records is uint32 [n, 8]: an inner record is {boxmin, hit}{boxmax, miss}, a TLAS leaf {objid, w2l_row, BLAS root link, flags}
        {meshid, hit, miss, twin}; links are typed byte offsets into the node image (device/scene_dev.hpp)."""
        n, root, base = C.c_uint32(0), C.c_int32(0), C.c_uint32(0)
        self._check(self._l.atn_tlas_download(self._ctx, None, 0, C.byref(n), C.byref(root), C.byref(base)))
        out = np.zeros((max(n.value, 1), 8), np.uint32)
        self._check(self._l.atn_tlas_download(self._ctx, out.ctypes.data, out.nbytes, C.byref(n), C.byref(root), C.byref(base)))
        return out[:n.value], int(root.value), int(base.value)

    def skin_buffer(self, skin, name):
        """For tests: "pos", "nml", "prev" (float32 [n, 4]), "bbox" (float32 [6]) or "area" (float32 [n_triangles])."""
        which = {"pos": 0, "nml": 1, "prev": 2, "bbox": 3, "area": 4}[name]
        nv, nt = self._skin_sizes.get(skin, (0, 0))
        out = np.zeros((max(nv, 1), 4), np.float32) if which < 3 else np.zeros(6 if which == 3 else max(nt, 1), np.float32)
        self._check(self._l.atn_skin_download(self._ctx, skin, which, out.ctypes.data))
        return out[:nv] if which < 3 else (out if which == 3 else out[:nt])

    def skin_scene_arrays(self, skin, n_vertices, n_triangles):
        """For tests: the whole scene on the device as new frames read it -- dict(shade float32 [T, 8, 4], vtx_pos / vtx_nml float32
        [V, 4], triangles TRIANGLE_PARAM [T]) for a scene of V vertices and T triangles."""
        out = dict(shade=np.zeros((n_triangles, 8, 4), np.float32), vtx_pos=np.zeros((n_vertices, 4), np.float32),
                   vtx_nml=np.zeros((n_vertices, 4), np.float32), triangles=np.zeros(n_triangles, L.TRIANGLE_PARAM))
        for which, k in ((5, "shade"), (6, "vtx_pos"), (7, "vtx_nml"), (8, "triangles")):
            self._check(self._l.atn_skin_download(self._ctx, skin, which, out[k].ctypes.data))
        return out

    def bvh_list_bytes(self, list_index):
        """For tests: the bytes of a bottom-level list in the device's node image, any-hit twins included."""
        n = C.c_uint32(0)
        self._check(self._l.atn_skin_download_list(self._ctx, list_index, None, 0, C.byref(n)))
        out = np.zeros(n.value, np.uint8)
        self._check(self._l.atn_skin_download_list(self._ctx, list_index, out.ctypes.data, n.value, C.byref(n)))
        return out

    def skin_close(self, skin):
        self._check(self._l.atn_skin_destroy(self._ctx, skin))
        self._skin_sizes.pop(skin, None)

    # ---- geometry motion vectors (docs/MOTION.md)
    def set_geometry_motion(self, on=True):
        """Keep the geometry history (the scene's vertex positions and matrices as the last compute_motion=2 frame saw them), so that
        svgf_render / restir_render accept compute_motion=2: motion vectors that follow skinned meshes and moved instances."""
        self._check(self._l.atn_set_geometry_motion(self._ctx, int(bool(on))))

    def geometry_motion_stats(self):
        """dict(passes, copies, copied_float4): motion passes run, range copies into the history, float4s they moved."""
        s = np.zeros(3, np.uint64)
        self._check(self._l.atn_geometry_motion_stats(self._ctx, s.ctypes.data))
        return dict(passes=int(s[0]), copies=int(s[1]), copied_float4=int(s[2]))

    def geometry_motion_matrices(self):
        """(w2c, prev_w2c) float32 [4, 4]: the camera matrices the last compute_motion=2 frame's motion pass used."""
        a, b = np.zeros((4, 4), np.float32), np.zeros((4, 4), np.float32)
        self._check(self._l.atn_geometry_motion_matrices(self._ctx, a.ctypes.data, b.ctypes.data))
        return a, b

    def scene_device_arrays(self):
        """(vtx_pos, vtx_nml, triangles) device addresses of the uploaded scene."""
        p = [C.c_void_p() for _ in range(3)]
        self._check(self._l.atn_scene_device_arrays(self._ctx, C.byref(p[0]), C.byref(p[1]), C.byref(p[2])))
        return tuple(x.value for x in p)

    def updateCamera(self, cam):
        self._check(self._l.atn_update_camera(self._ctx, cam.ctypes.data))

    def initSampler(self, width, height, seed=0):
        self._check(self._l.atn_init_sampler(self._ctx, width, height, seed))

    def setRandom(self, seeds):
        seeds = np.ascontiguousarray(seeds, np.uint32)
        self._check(self._l.atn_set_random(self._ctx, seeds.ctypes.data, len(seeds)))

    def getRandom(self):
        out = np.zeros(self._l.atn_random_count(self._ctx), np.uint32)
        if len(out):
            self._check(self._l.atn_get_random(self._ctx, out.ctypes.data, len(out)))
        return out

    def setScreenShard(self, rank, world):
        self._check(self._l.atn_set_screen_shard(self._ctx, rank, world))

    def render(self, width, height, max_depth=5, rr_depth=3, spp=1, frame=0, progressive=True,
               break_on_terminate=True, download=True, count_stats=False, profile=False):
        d = Destination(width, height, max_depth, rr_depth, spp, frame, int(progressive),
                        int(break_on_terminate), int(count_stats), int(profile))
        out = np.empty((height, width, 4), np.float32) if download else None
        self._check(self._l.atn_render(self._ctx, C.byref(d), out.ctypes.data if download else None))
        self.width, self.height = width, height
        return out

    def set_upload_options(self, anyhit_twin=None, anyhit_twin_dirs=None, node_layout=None, planar_lights=None):
        """How the next UpdateSceneData lays the scene out (atn_set_upload_options); None leaves an option as it is."""
        v = lambda x: -1 if x is None else int(x)
        self._check(self._l.atn_set_upload_options(self._ctx, v(anyhit_twin), v(anyhit_twin_dirs), v(node_layout), v(planar_lights)))

    def set_sphere_intersection(self, mode):
        """Analytic spheres (docs/SPHERES.md): 0 (default) a sphere object's top-layer leaf is never tested, as in the CPU tracer; 1 the
        next UpdateSceneData / update_tlas makes such leaves records every ray tests with sphere::hit."""
        self._check(self._l.atn_set_sphere_intersection(self._ctx, int(mode)))

    def sphere_leaves(self):
        """How many top-layer leaves of the uploaded scene are tested as spheres (0 in mode 0)."""
        n = C.c_uint32(0)
        self._check(self._l.atn_sphere_leaves(self._ctx, C.byref(n)))
        return int(n.value)

    def set_shade_math(self, relaxed):
        """False (default): the parity path; True: the shade kernel under the reference GPU build's --use_fast_math rules (opt-in)."""
        self._check(self._l.atn_set_shade_math(self._ctx, int(relaxed)))

    def set_rr_lookahead(self, mode):
        """The roulette look-ahead of render() (include/aten_amd.h): 0 off, 1 on where the scene qualifies (default; counted frames
        keep the reference's accounting), 2 counted frames too (rr_lookahead_stats).  Films are byte-equal in every mode."""
        self._check(self._l.atn_set_rr_lookahead(self._ctx, int(mode)))

    def rr_lookahead_active(self):
        """Whether frames of the current scene run the look-ahead (no emissive, singular, translucent, CarPaint or toon material)."""
        return bool(self._l.atn_rr_lookahead_active(self._ctx))

    def rr_lookahead_stats(self):
        """Of the last counted frame in mode 2: the rays traced as any-hit rays, their hits (ended unshaded), their visits."""
        s = np.zeros(4, np.uint64)
        self._check(self._l.atn_rr_lookahead_stats(self._ctx, s.ctypes.data))
        return dict(doomed_rays=int(s[0]), doomed_hits=int(s[1]), doomed_nodes=int(s[2]), doomed_tris=int(s[3]))

    def set_nee_deferral(self, mode):
        """The deferred NEE of render() (include/aten_amd.h): 0 off (the mode a context starts in), 1 on wherever the scene qualifies, 2 (the
        policy) where it qualifies and every light is infinite.  Films are byte-equal in every mode."""
        self._check(self._l.atn_set_nee_deferral(self._ctx, int(mode)))

    def nee_deferral_active(self):
        """Whether frames of the current scene defer their NEE evaluation under the current mode."""
        return bool(self._l.atn_nee_deferral_active(self._ctx))

    def nee_deferral_stats(self):
        """Over the deferred frames since the last reset(): shadow rays cast and the ones that reached their light."""
        s = np.zeros(2, np.uint64)
        self._check(self._l.atn_nee_deferral_stats(self._ctx, s.ctypes.data))
        return dict(cast=int(s[0]), reached=int(s[1]))

    def set_regeneration(self, on):
        """Path regeneration (include/aten_amd.h): the samples of a frame / the frames of a burst share one pool of path slots.
        Off by default.  Measured guidance: switch it on for render_burst of >= 2 multi-sample frames in the
        break-on-terminate sample loop (1080p 8 spp: 1.14-1.23 x over four serial frames in flight, 1.7-2.0 x for a caller with one
        frame in flight) and for one-frame-in-flight shards of scenes whose paths differ in length; leave it off at 1 spp with
        frames in flight and when every sample is traced (0.72-0.92 x)."""
        self._check(self._l.atn_set_regeneration(self._ctx, int(on)))

    def render_burst(self, width, height, n_frames, max_depth=5, rr_depth=3, spp=1, frame=0, progressive=True,
                     break_on_terminate=True, download=True, profile=False):
        """n_frames consecutive frames (frame, frame + 1, ...) in one call; the film after the last one."""
        d = Destination(width, height, max_depth, rr_depth, spp, frame, int(progressive), int(break_on_terminate), 0, int(profile))
        out = np.empty((height, width, 4), np.float32) if download else None
        self._check(self._l.atn_render_burst(self._ctx, C.byref(d), n_frames, out.ctypes.data if download else None))
        self.width, self.height = width, height
        return out

    def regen_stage_counts(self):
        """(closest-hit rays, shadow rays) per launch of the last regenerated burst."""
        n = C.c_uint32(0)
        self._check(self._l.atn_regen_stage_counts(self._ctx, None, None, 0, C.byref(n)))
        q = np.zeros(n.value, np.uint32); sh = np.zeros(n.value, np.uint32)
        if n.value:
            self._check(self._l.atn_regen_stage_counts(self._ctx, q.ctypes.data, sh.ctypes.data, n.value, C.byref(n)))
        return q, sh

    def set_path_batches(self, n):
        self._check(self._l.atn_set_path_batches(self._ctx, n))

    def set_frames_in_flight(self, n):
        self._check(self._l.atn_set_frames_in_flight(self._ctx, n))

    def side_stream_ptr(self):
        """hipStream_t for the caller's own work beside the frames in flight (atn_side_stream)"""
        p = self._l.atn_side_stream(self._ctx)
        if not p:
            raise AtenAmdError("atn_side_stream failed")
        return p

    def bank_streams(self):
        """(streams replaced by the queue probe so far, every pair of bank streams measured to run side by side)"""
        sw, cc = C.c_int32(0), C.c_int32(0)
        self._check(self._l.atn_bank_streams(self._ctx, C.byref(sw), C.byref(cc)))
        self.side_stream_concurrent = bool(cc.value & 2)    # the side stream (if handed out) runs beside every bank stream
        return sw.value, bool(cc.value & 1)

    def set_sampling_options(self, ibl_importance=False, tex_bilinear=False):
        self._check(self._l.atn_set_sampling_options(self._ctx, int(ibl_importance), int(tex_bilinear)))

    def sample_texture(self, texid, uv):
        uv = np.ascontiguousarray(uv, np.float32).reshape(-1, 2)
        out = np.zeros((len(uv), 4), np.float32)
        self._check(self._l.atn_sample_texture(self._ctx, texid, len(uv), uv.ctypes.data, out.ctypes.data))
        return out

    def reset(self):
        self._check(self._l.atn_reset(self._ctx))

    # ---- results / instrumentation
    def synchronize(self):
        self._check(self._l.atn_synchronize(self._ctx))

    def film_device_ptr(self):
        return self._l.atn_film_device(self._ctx)

    def tile_device_ptr(self):
        return self._l.atn_tile_device(self._ctx)

    def tile_slots(self):
        return int(self._l.atn_tile_slots(self._ctx))

    def stream_ptr(self):
        return self._l.atn_stream(self._ctx)

    def assemble_tiles(self, gathered_dev_ptr, world, out_dev_ptr=None, stream_ptr=None):
        self._check(self._l.atn_assemble_tiles_on(self._ctx, gathered_dev_ptr, world, out_dev_ptr, stream_ptr))

    def download_film(self):
        out = np.empty((self.height, self.width, 4), np.float32)
        self._check(self._l.atn_download_film(self._ctx, out.ctypes.data))
        return out

    def upload_film(self, film):
        """Resume from a film returned by download_film / render (running mean + sample count)."""
        film = np.ascontiguousarray(film, np.float32)
        h, w = film.shape[:2]
        self._check(self._l.atn_upload_film(self._ctx, w, h, film.ctypes.data))
        self.width, self.height = w, h

    def path_cost(self):
        """uint32 [h, w, 2]: BVH node visits and triangle tests per pixel of the last frame rendered with count_stats=True."""
        out = np.zeros((self.height, self.width, 2), np.uint32)
        self._check(self._l.atn_download_path_cost(self._ctx, out.ctypes.data))
        return out

    def anyhit_twins(self):
        """atn_anyhit_twins: bottom-level lists that have an any-hit twin right now."""
        return int(self._l.atn_anyhit_twins(self._ctx))

    def planar_area_lights(self):
        """atn_planar_area_lights: area lights whose shadow rays may stop at the first hit nearer than the light."""
        return int(self._l.atn_planar_area_lights(self._ctx))

    def stats(self):
        s = np.zeros(8, np.uint64)
        self._check(self._l.atn_get_stats(self._ctx, s.ctypes.data))
        return dict(closest_rays=int(s[0]), shadow_rays=int(s[1]), hits=int(s[2]),
                    closest_nodes=int(s[3]), closest_tris=int(s[4]), shadow_nodes=int(s[5]), shadow_tris=int(s[6]))

    # ---- SVGF (aten::SVGFRenderer)
    SVGF_BUFFERS = dict(normal_depth=0, albedo_meshid=1, color_variance=2, moment_temporalweight=3,
                        prev_normal_depth=4, prev_albedo_meshid=5, prev_color_variance=6, prev_moment_temporalweight=7,
                        temporary_color=8, motion_depth=9, primary_position=10, atrous0=11, atrous1=12, output=13,
                        contribs=14, primary_hit=15)

    def svgf_render(self, width, height, max_depth=5, rr_depth=3, spp=1, frame=0, compute_motion=False, stages=False,
                    download=True, profile=False):
        """SVGFRenderer::OnRender.  Returns the filtered frame [h, w, 4] (and the three intermediate puts)."""
        d = Destination(width, height, max_depth, rr_depth, spp, frame, 0, 1, 0, int(profile))
        out = np.empty((height, width, 4), np.float32) if download else None
        st = np.empty((3, height, width, 4), np.float32) if stages else None
        self._check(self._l.atn_svgf_render(self._ctx, C.byref(d), int(compute_motion),
                                            out.ctypes.data if download else None, st.ctypes.data if stages else None))
        self.width, self.height = width, height
        return (out, st) if stages else out

    # ---- ReSTIR (idaten::ReSTIRPathTracing: UpdateSceneData / SetGBuffer / render; docs/RESTIR.md)
    RESTIR_MODES = {"initial": 0, "restir": 1, "spatial": 2, "temporal": 3}
    RESTIR_STAGES = {"initial": 0, "temporal": 1, "spatial": 2}

    def restir_set_options(self, mode=1, n_candidates=32):
        """mode 0 = initial candidates only, 1 = temporal + spatial (default), 2 = spatial, 3 = temporal; n_candidates in [1, 32]."""
        self._check(self._l.atn_restir_set_options(self._ctx, self.RESTIR_MODES.get(mode, mode), n_candidates))

    def restir_render(self, width, height, max_depth=5, rr_depth=3, frame=0, progressive=True, compute_motion=False,
                      download=True, profile=False):
        """One ReSTIR frame (1 sample per pixel) into the film; returns the film [h, w, 4]."""
        d = Destination(width, height, max_depth, rr_depth, 1, frame, int(progressive), 1, 0, int(profile))
        out = np.empty((height, width, 4), np.float32) if download else None
        self._check(self._l.atn_restir_render(self._ctx, C.byref(d), int(compute_motion), out.ctypes.data if download else None))
        self.width, self.height = width, height
        return out

    def restir_set_motion_depth(self, md):
        md = np.ascontiguousarray(md, np.float32).reshape(-1, 4)
        self._check(self._l.atn_restir_set_motion_depth(self._ctx, md.ctypes.data, len(md)))

    def restir_reset(self):
        self._check(self._l.atn_restir_reset(self._ctx))

    def restir_capture(self, on=True):
        """Keep the stage buffers (reservoirs after each pass, CMJ dimensions) of the next frames for restir_buffer."""
        self._check(self._l.atn_restir_capture(self._ctx, int(on)))

    def restir_buffer(self, name):
        """The last ReSTIR frame's stage buffers.  'initial' / 'temporal' / 'spatial': dict of [h, w] arrays y, M (int32), W, w_sum,
        target_pdf (needs restir_capture); 'info': dict nml, wi, p [h, w, 3], u, v, pre_r, mtrl, mesh, hit; 'nd' / 'am' / 'motion':
        [h, w, 4]; 'dims': uint32 [h, w] (needs restir_capture); 'primary_hit': the ids plane [h, w, 4] of a frame rendered with
        compute_motion=2 (unpack_primary_hit)."""
        w, h = self.width, self.height
        if name in self.RESTIR_STAGES:
            out = np.empty((h, w, 5), np.float32)
            self._check(self._l.atn_restir_download(self._ctx, self.RESTIR_STAGES[name], out.ctypes.data))
            return dict(y=out[..., 0].astype(np.int32), M=out[..., 1].astype(np.int32), W=out[..., 2].copy(),
                        w_sum=out[..., 3].copy(), target_pdf=out[..., 4].copy())
        if name == "info":
            out = np.empty((4, h, w, 4), np.float32)
            self._check(self._l.atn_restir_download(self._ctx, 3, out.ctypes.data))
            return dict(nml=out[0, ..., :3].copy(), mtrl=out[0, ..., 3].copy().view(np.int32), wi=out[1, ..., :3].copy(),
                        u=out[1, ..., 3].copy(), p=out[2, ..., :3].copy(), v=out[2, ..., 3].copy(), pre_r=out[3, ..., 0].copy(),
                        mesh=out[3, ..., 1].copy().view(np.int32), hit=out[3, ..., 2].copy())
        if name == "dims":
            out = np.empty((h, w), np.uint32)
            self._check(self._l.atn_restir_download(self._ctx, 7, out.ctypes.data))
            return out
        which = {"nd": 4, "am": 5, "motion": 6, "primary_hit": 8}[name]
        out = np.empty((h, w, 4), np.float32)
        self._check(self._l.atn_restir_download(self._ctx, which, out.ctypes.data))
        return out

    # ---- NPR feature lines (idaten::NPRPathTracing / aten::NprPathTracer; docs/NPR.md)
    def npr_render(self, width, height, max_depth=5, rr_depth=3, spp=1, frame=0, progressive=True, break_on_terminate=True,
                   download=True, profile=False):
        """One frame with feature lines (the scene's FeatureLineConfig must be enabled) into the film; returns the film [h, w, 4]."""
        d = Destination(width, height, max_depth, rr_depth, spp, frame, int(progressive), int(break_on_terminate), 0, int(profile))
        out = np.empty((height, width, 4), np.float32) if download else None
        self._check(self._l.atn_npr_render(self._ctx, C.byref(d), out.ctypes.data if download else None))
        self.width, self.height = width, height
        return out

    def npr_reset(self):
        """Film and sample-ray state of a fresh context."""
        self._check(self._l.atn_npr_reset(self._ctx))

    def npr_capture(self, on=True):
        """Keep the stage buffers (line decision, sample-ray descriptors, disc, CMJ dimension) of the next frames for npr_buffer."""
        self._check(self._l.atn_npr_capture(self._ctx, int(on)))

    def npr_buffer(self, name):
        """The last NPR frame's stage buffers (needs npr_capture).  'line': dict found (bool), bounce (int32), distance [h, w];
        'desc': dict u, v, live [h, w, 8] after bounce 0; 'disc': dict center [h, w, 3], radius, normal [h, w, 3], acc after
        bounce 0; 'dims': uint32 [h, w], the CMJ dimension after bounce 0."""
        w, h = self.width, self.height
        if name == "line":
            out = np.empty((h, w, 4), np.float32)
            self._check(self._l.atn_npr_download(self._ctx, 0, out.ctypes.data))
            return dict(found=out[..., 0] != 0, bounce=out[..., 1].astype(np.int32), distance=out[..., 2].copy())
        if name == "desc":
            out = np.empty((h, w, 8, 4), np.float32)
            self._check(self._l.atn_npr_download(self._ctx, 1, out.ctypes.data))
            return dict(u=out[..., 0].copy(), v=out[..., 1].copy(), live=out[..., 2] != 0)
        if name == "disc":
            out = np.empty((h, w, 2, 4), np.float32)
            self._check(self._l.atn_npr_download(self._ctx, 2, out.ctypes.data))
            return dict(center=out[..., 0, :3].copy(), radius=out[..., 0, 3].copy(), normal=out[..., 1, :3].copy(), acc=out[..., 1, 3].copy())
        if name == "dims":
            out = np.empty((h, w), np.uint32)
            self._check(self._l.atn_npr_download(self._ctx, 3, out.ctypes.data))
            return out
        raise ValueError("no NPR buffer %r" % (name,))

    def npr_set_skip_through(self, mode):
        """0 (default): npr_render refuses STENCIL materials and alpha blending with an alpha that may be < 1; 1: it looks through them
        (AdvanceNPRPath: CheckStencil, CheckMaterialTranslucentByAlpha; docs/NPR_ADVANCE.md)."""
        self._check(self._l.atn_npr_set_skip_through(self._ctx, int(mode)))

    def npr_advance_buffer(self):
        """The look-through's stage of the last NPR frame after bounce 0 (needs npr_capture, npr_set_skip_through(1) and a scene that
        looks through something): dict kind (0 none, 1 stencil, 2 alpha), walks, answer (triangle id, -1 = miss) int32 [h, w],
        singular bool [h, w], throughput float32 [h, w, 3], transmission float32 [h, w]."""
        w, h = self.width, self.height
        out = np.empty((h, w, 2, 4), np.float32)
        self._check(self._l.atn_npr_advance_download(self._ctx, out.ctypes.data))
        return dict(kind=out[..., 0, 0].astype(np.int32), walks=out[..., 0, 1].astype(np.int32), answer=out[..., 0, 2].astype(np.int32),
                    singular=out[..., 0, 3] != 0, throughput=out[..., 1, :3].copy(), transmission=out[..., 1, 3].copy())

    # ---- volume rendering: path tracing through homogeneous and grid media (aten::VolumePathTracing; docs/VOLUME.md)
    def volume_set_grids(self, grids):
        """The dense grids a medium names by grid_idx (SceneBuilder.add_medium_material(grid=...)): a list of
        (density float32 [z, y, x], origin (x, y, z), voxel_size), copied; [] drops them.  A built scene carries its own as
        FlatScene.grids.  They outlive the update_* edits; upload_scene drops them."""
        grids = list(grids)
        arr = (VolumeGrid * max(1, len(grids)))()
        keep = []
        for i, (density, origin, voxel_size) in enumerate(grids):
            d = np.ascontiguousarray(density, np.float32)
            if d.ndim != 3:
                raise ValueError("a grid's density is an array [z, y, x]")
            keep.append(d)
            arr[i].dim[:] = [d.shape[2], d.shape[1], d.shape[0]]
            arr[i].origin[:] = [float(c) for c in origin]
            arr[i].voxel_size = float(voxel_size)
            arr[i].density = d.ctypes.data
        self._check(self._l.atn_volume_set_grids(self._ctx, C.byref(arr) if grids else None, len(grids)))

    def volume_render(self, width, height, max_depth=5, rr_depth=3, spp=1, frame=0, progressive=True, break_on_terminate=True,
                      download=True, profile=False):
        """One frame through the scene's media (materials with is_medium set) into the film; returns the film [h, w, 4]."""
        d = Destination(width, height, max_depth, rr_depth, spp, frame, int(progressive), int(break_on_terminate), 0, int(profile))
        out = np.empty((height, width, 4), np.float32) if download else None
        self._check(self._l.atn_volume_render(self._ctx, C.byref(d), out.ctypes.data if download else None))
        self.width, self.height = width, height
        return out

    def volume_reset(self):
        """The film of a fresh context."""
        self._check(self._l.atn_volume_reset(self._ctx))

    def volume_capture(self, iteration=0):
        """Keep the per-pixel state after `iteration` (0..7) of sample 0 of the next frames for volume_buffer; None or < 0: off."""
        self._check(self._l.atn_volume_capture(self._ctx, -1 if iteration is None else int(iteration)))

    def volume_buffer(self, name):
        """The last volume frame's stage buffers (needs volume_capture, except 'counters').  'state': dict of bool [h, w] processed,
        hit, sampled, absorbed, scattered, passed, connection, terminated and int32 depth_count, stack_size, uint32 dim;
        'stack': int32 [h, w, 8], the medium stack in the order entered (entries beyond stack_size are 0);
        'ray': dict org [h, w, 3], dir [h, w, 3], s, hit_t; 'conn': dict org, dir, t_max, transmittance, segments (int32), visible;
        'counters': dict stack_overflow, walk_overflow, connections, segments of the last frame;
        'grid_counters': dict flight_capped, connection_capped: grid flights / connections stopped after 16384 tracking steps.
        With grid media 'state' has flight_steps (the delta-tracking steps of the flight), and 'conn' track_steps and stream_dim (the
        ratio-tracking steps and the final dimension of the connection's own sample stream)."""
        w, h = self.width, self.height
        if name == "counters":
            out = np.zeros(4, np.uint32)
            self._check(self._l.atn_volume_download(self._ctx, 4, out.ctypes.data))
            return dict(stack_overflow=int(out[0]), walk_overflow=int(out[1]), connections=int(out[2]), segments=int(out[3]))
        if name == "grid_counters":
            out = np.zeros(2, np.uint32)
            self._check(self._l.atn_volume_download(self._ctx, 5, out.ctypes.data))
            return dict(flight_capped=int(out[0]), connection_capped=int(out[1]))
        if name == "state":
            out = np.empty((h, w, 4), np.uint32)
            self._check(self._l.atn_volume_download(self._ctx, 0, out.ctypes.data))
            return unpack_volume_state(out)
        if name == "stack":
            st = np.empty((h, w, 4), np.uint32)
            self._check(self._l.atn_volume_download(self._ctx, 0, st.ctypes.data))
            out = np.empty((h, w, 4), np.uint32)
            self._check(self._l.atn_volume_download(self._ctx, 1, out.ctypes.data))
            return unpack_volume_stack(out, st[..., 2])
        if name == "ray":
            out = np.empty((h, w, 2, 4), np.float32)
            self._check(self._l.atn_volume_download(self._ctx, 2, out.ctypes.data))
            return dict(org=out[..., 0, :3].copy(), s=out[..., 0, 3].copy(), dir=out[..., 1, :3].copy(), hit_t=out[..., 1, 3].copy())
        if name == "conn":
            out = np.empty((h, w, 3, 4), np.float32)
            self._check(self._l.atn_volume_download(self._ctx, 3, out.ctypes.data))
            return dict(org=out[..., 0, :3].copy(), t_max=out[..., 0, 3].copy(), dir=out[..., 1, :3].copy(), transmittance=out[..., 1, 3].copy(),
                        segments=out[..., 2, 0].astype(np.int32), visible=out[..., 2, 1] != 0,
                        track_steps=out[..., 2, 2].astype(np.int32), stream_dim=out[..., 2, 3].astype(np.int32))
        raise ValueError("no volume buffer %r" % (name,))

    def volume_phase_table(self, g, w, r1, r2, wo):
        """HenyeyGreensteinPhaseFunction on the device for n cases: (SampleDirection(r1, r2, g, w) [n, 3], Evaluate(g, w, wo) [n])."""
        w = np.ascontiguousarray(w, np.float32).reshape(-1, 3)
        wo = np.ascontiguousarray(wo, np.float32).reshape(-1, 3)
        r1 = np.ascontiguousarray(r1, np.float32).reshape(-1)
        r2 = np.ascontiguousarray(r2, np.float32).reshape(-1)
        n = len(r1)
        assert len(w) == n and len(wo) == n and len(r2) == n
        out_dir = np.empty((n, 3), np.float32)
        out_eval = np.empty(n, np.float32)
        self._check(self._l.atn_volume_phase_table(self._ctx, float(g), n, w.ctypes.data, r1.ctypes.data, r2.ctypes.data, wo.ctypes.data,
                                                   out_dir.ctypes.data, out_eval.ctypes.data))
        return out_dir, out_eval

    # ---- ambient occlusion (aten::AORenderer / idaten::AORenderer; docs/AO.md)
    def ao_set_params(self, num_rays=1, radius=1.0, filter=False):
        """AO rays per pixel (1..64), their radius, and whether the depth-aware bilateral filter runs (AORenderer's defaults)."""
        self._check(self._l.atn_ao_set_params(self._ctx, int(num_rays), float(radius), int(filter)))

    def ao_render(self, width, height, frame=0, progressive=True, break_on_terminate=True, download=True, profile=False, count_stats=False):
        """One AO frame into the film; returns the film [h, w, 4].  break_on_terminate=True is the CPU renderer as written: in every
        row the pixels from the first primary miss on are not written (the Cornell box at 4:3 misses at x = 0 of every row: nothing is
        written); False is idaten's rule: a primary miss is 1.0 and every pixel is written."""
        d = Destination(width, height, 1, 1, 1, frame, int(progressive), int(break_on_terminate), int(count_stats), int(profile))
        out = np.empty((height, width, 4), np.float32) if download else None
        self._check(self._l.atn_ao_render(self._ctx, C.byref(d), out.ctypes.data if download else None))
        self.width, self.height = width, height
        return out

    def ao_reset(self):
        """Film and AO planes of a fresh context."""
        self._check(self._l.atn_ao_reset(self._ctx))

    def ao_capture(self, on=True):
        """Keep the first AO ray and its answer of the next frames for ao_buffer('ray' / 'answer')."""
        self._check(self._l.atn_ao_capture(self._ctx, int(on)))

    def ao_buffer(self, name):
        """The last AO frame's planes.  'state': uint32 [h, w], 0 not rendered / 1 hit / 2 miss; 'value': float32 [h, w], the AO value
        handed to the film (before the filter); 'depth': float32 [h, w], the primary hit's t (inf: a miss); 'first_miss': int64 [h], the
        row's first primary miss x (width: none).  With ao_capture: 'ray': dict org, dir [h, w, 3] of the pixel's first AO ray;
        'answer': dict kind (0 miss / 1 hit / 2 ten skip-throughs), t, c, skips [h, w] of that ray (pixels in state 1)."""
        w, h = self.width, self.height
        if name in ("state", "value", "depth"):
            out = np.empty((h, w), np.uint32 if name == "state" else np.float32)
            self._check(self._l.atn_ao_download(self._ctx, ("state", "value", "depth").index(name), out.ctypes.data))
            return out
        if name == "first_miss":
            out = np.empty(h, np.uint32)
            self._check(self._l.atn_ao_download(self._ctx, 3, out.ctypes.data))
            return np.minimum(out.astype(np.int64), w)
        if name == "ray":
            out = np.empty((h, w, 2, 4), np.float32)
            self._check(self._l.atn_ao_download(self._ctx, 4, out.ctypes.data))
            return dict(org=out[..., 0, :3].copy(), dir=out[..., 1, :3].copy())
        if name == "answer":
            out = np.empty((h, w, 4), np.float32)
            self._check(self._l.atn_ao_download(self._ctx, 5, out.ctypes.data))
            return dict(kind=out[..., 0].astype(np.int32), t=out[..., 1].copy(), c=out[..., 2].copy(), skips=out[..., 3].astype(np.int32))
        raise ValueError("no AO buffer %r" % (name,))

    # ---- the NPR shadow pre-pass (NprPathTracer::OnRender's first pass / idaten's onShadeByShadowRay; docs/NPR_SHADOW.md)
    def set_npr_shadow(self, mode):
        """0 (default): Toon shading reads the screen-space shadow texture uploaded with the scene; 1: render() and npr_render() first
        make it from the frame's own bounce-0 shadow rays (the depth-aware row filter over "the ray reached its light")."""
        self._check(self._l.atn_npr_shadow_set_mode(self._ctx, int(mode)))

    def npr_shadow_buffer(self, which):
        """The planes of the last frame that ran the pre-pass, float32 [h, w]: 'plane' / 0 the filtered plane, 'lit' / 1 the bit as
        0.0 / 1.0, 'depth' / 2 the primary hit's t (inf: a miss)."""
        k = ("plane", "lit", "depth").index(which) if isinstance(which, str) else int(which)
        out = np.empty((self.height, self.width), np.float32)
        self._check(self._l.atn_npr_shadow_download(self._ctx, k, out.ctypes.data, out.size))
        return out

    def npr_shadow_filter(self, lit, depth):
        """The pre-pass's row filter alone over host planes [h, w] (11 taps, ApplyBilateralFilter<ShadowRay, float, true, 5>)."""
        l = np.ascontiguousarray(lit, np.float32)
        d = np.ascontiguousarray(depth, np.float32)
        if l.shape != d.shape or l.ndim != 2:
            raise ValueError("lit and depth are [h, w] planes of one shape")
        out = np.empty_like(l)
        self._check(self._l.atn_npr_shadow_filter(self._ctx, l.ctypes.data, d.ctypes.data, l.shape[1], l.shape[0], out.ctypes.data))
        return out

    # ---- NPR hatching shadows (idaten::NPRPathTracing's HatchingShadowBase x HatchingShadowDirection; docs/NPR_HATCHING.md)
    HATCH_BASES = ("ao", "shadow_ray")
    HATCH_DIRECTIONS = ("none", "horizontal", "vertical", "orthogonal", "cross", "orthogonal_cross")

    def set_npr_hatching(self, base=1, direction=1, ao_num_rays=1, ao_radius=1.0):
        """What the mode-1 pre-pass filters and how.  base: 0 / 'ao' the AO value at the primary hit (ao_num_rays rays of ao_radius),
        1 / 'shadow_ray' the bounce-0 lit bit (default).  direction: 0..5 or a name of HATCH_DIRECTIONS (default 1, the row)."""
        b = self.HATCH_BASES.index(base) if isinstance(base, str) else int(base)
        d = self.HATCH_DIRECTIONS.index(direction) if isinstance(direction, str) else int(direction)
        self._check(self._l.atn_npr_hatching_set(self._ctx, b, d, int(ao_num_rays), float(ao_radius)))

    def npr_hatching(self):
        """The settings: dict base, direction, ao_num_rays, ao_radius."""
        b, d, n, r = C.c_int32(), C.c_int32(), C.c_int32(), C.c_float()
        self._check(self._l.atn_npr_hatching_get(self._ctx, C.byref(b), C.byref(d), C.byref(n), C.byref(r)))
        return dict(base=b.value, direction=d.value, ao_num_rays=n.value, ao_radius=r.value)

    def npr_hatching_buffer(self, which):
        """Planes of the last frame that ran the pre-pass, float32 [h, w]: 'source' / 0 what was filtered (AO values, or the bit as
        0.0 / 1.0), 'first' / 1 the first step's plane (the final plane of a one-step direction)."""
        k = ("source", "first").index(which) if isinstance(which, str) else int(which)
        out = np.empty((self.height, self.width), np.float32)
        self._check(self._l.atn_npr_hatching_download(self._ctx, k, out.ctypes.data, out.size))
        return out

    def npr_hatching_filter(self, src, depth, direction):
        """The filter of one direction alone over host planes [h, w]."""
        s = np.ascontiguousarray(src, np.float32)
        d = np.ascontiguousarray(depth, np.float32)
        if s.shape != d.shape or s.ndim != 2:
            raise ValueError("src and depth are [h, w] planes of one shape")
        k = self.HATCH_DIRECTIONS.index(direction) if isinstance(direction, str) else int(direction)
        out = np.empty_like(s)
        self._check(self._l.atn_npr_hatching_filter(self._ctx, s.ctypes.data, d.ctypes.data, s.shape[1], s.shape[0], k, out.ctypes.data))
        return out

    def svgf_denoise(self, width, height, frame=0, compute_motion=False, stages=False, download=True, profile=False):
        """The filter passes of OnRender on the buffers as they stand (svgf_upload / a previous path pass)."""
        d = Destination(width, height, 1, 1, 1, frame, 0, 1, 0, int(profile))
        out = np.empty((height, width, 4), np.float32) if download else None
        st = np.empty((3, height, width, 4), np.float32) if stages else None
        self._check(self._l.atn_svgf_denoise(self._ctx, C.byref(d), int(compute_motion),
                                             out.ctypes.data if download else None, st.ctypes.data if stages else None))
        self.width, self.height = width, height
        return (out, st) if stages else out

    def svgf_upload(self, name, data):
        data = np.ascontiguousarray(data, np.float32)
        h, w = data.shape[:2]
        self._check(self._l.atn_svgf_upload(self._ctx, self.SVGF_BUFFERS[name], w, h, data.ctypes.data))
        self.width, self.height = w, h

    def svgf_set_motion_depth(self, md):
        md = np.ascontiguousarray(md, np.float32).reshape(-1, 4)
        self._check(self._l.atn_svgf_set_motion_depth(self._ctx, md.ctypes.data, len(md)))

    def svgf_reset(self):
        self._check(self._l.atn_svgf_reset(self._ctx))

    def svgf_set_dilate_temporal_weight(self, on):
        self._check(self._l.atn_svgf_set_dilate_temporal_weight(self._ctx, int(on)))

    def svgf_set_atrous_iterations(self, n):
        self._check(self._l.atn_svgf_set_atrous_iterations(self._ctx, n))

    def svgf_buffer(self, name):
        """A buffer of the last SVGF frame, float32 [h, w, 4] (SVGF_BUFFERS).  'primary_hit' is the ids plane of a frame rendered with
        compute_motion=2: object id and triangle id as int bits, a, b (unpack_primary_hit)."""
        out = np.empty((self.height, self.width, 4), np.float32)
        self._check(self._l.atn_svgf_download(self._ctx, self.SVGF_BUFFERS[name], out.ctypes.data))
        return out

    # ---- the display tail: temporal anti-aliasing + gamma (docs/TAA.md) ----
    TAA_SOURCES = {"svgf": 0, "restir": 1, "uploaded": 2}
    TAA_UPLOADS = {"color": 0, "motion_depth": 1, "history": 2}
    TAA_BUFFERS = {"output": 0, "previous_history": 1, "gamma": 2, "rgba8": 3}

    def taa_resolve(self, width, height, source="svgf", enable=True, gamma=2.2, want_float=False, want_rgba8=False):
        """aten::TAA + aten::GammaCorrection behind the last frame of `source` ('svgf', 'restir', or 'uploaded': the planes of
        taa_upload), one kernel launch.  Without want_*: enqueued, no host wait, returns None (the results stay on the device:
        taa_buffer, atn_taa_output_device).  want_float: the gamma plane float32 [h, w, 4]; want_rgba8: uint8 [h, w, 4] (R, G, B, A)."""
        gf = np.empty((height, width, 4), np.float32) if want_float else None
        g8 = np.empty((height, width), np.uint32) if want_rgba8 else None
        self._check(self._l.atn_taa_resolve(self._ctx, self.TAA_SOURCES[source], width, height, int(bool(enable)), float(gamma),
                                            gf.ctypes.data if want_float else None, g8.ctypes.data if want_rgba8 else None))
        self._taa_size = (height, width)
        if want_rgba8:
            g8 = g8.view(np.uint8).reshape(height, width, 4)
        return (gf, g8) if (want_float and want_rgba8) else gf if want_float else g8

    def taa_upload(self, name, data):
        """'color' / 'motion_depth' (source 'uploaded') or 'history', float32 [h, w, 4], row 0 = bottom."""
        data = np.ascontiguousarray(data, np.float32)
        h, w = data.shape[:2]
        self._check(self._l.atn_taa_upload(self._ctx, self.TAA_UPLOADS[name], w, h, data.ctypes.data))

    def taa_buffer(self, name):
        """Of the last taa_resolve: 'output' (= the new history), 'previous_history', 'gamma' (float32 [h, w, 4]; needs want_float) or
        'rgba8' (uint8 [h, w, 4])."""
        h, w = self._taa_size
        which = self.TAA_BUFFERS[name]
        out = np.empty((h, w), np.uint32) if which == 3 else np.empty((h, w, 4), np.float32)
        self._check(self._l.atn_taa_download(self._ctx, which, out.ctypes.data))
        return out.view(np.uint8).reshape(h, w, 4) if which == 3 else out

    def taa_reset(self):
        self._check(self._l.atn_taa_reset(self._ctx))

    def kernel_times(self):
        ms = np.zeros(len(K_NAMES), np.float32); n = np.zeros(len(K_NAMES), np.uint32)
        self._check(self._l.atn_get_kernel_times(self._ctx, ms.ctypes.data, n.ctypes.data))
        return {k: (float(ms[i]), int(n[i])) for i, k in enumerate(K_NAMES)}

    def reset_kernel_times(self):
        self._check(self._l.atn_reset_kernel_times(self._ctx))

    # ---- stage entry points (parity tests)
    def generate_paths(self, width, height, sample=0, frame=0):
        rays = np.zeros(width * height, L.RAY)
        self._check(self._l.atn_generate_paths(self._ctx, width, height, sample, frame, rays.ctypes.data))
        return rays

    def trace_closest(self, rays, t_min=1e-9, t_max=float(np.finfo(np.float32).max), stats=False):
        rays = np.ascontiguousarray(rays)
        out = np.zeros(len(rays), L.INTERSECTION)
        st = np.zeros(2, np.uint64)
        self._check(self._l.atn_trace_closest(self._ctx, rays.ctypes.data, len(rays), t_min, t_max,
                                              out.ctypes.data, st.ctypes.data if stats else None))
        return (out, st) if stats else out

    SHADOW_FLAVOURS = {"fused": 0, "counted": 1, "deferred": 2, "regen": 3}

    def trace_shadow(self, origins, directions, dist_to_light, light, stencil_always=False, flavour="fused", final=None):
        """HitShadowRay's verdict for n caller-given shadow rays through the production shadow kernels (atn_trace_shadow): origins and
        directions [n, 3] (directions need not be unit length), dist_to_light [n], light [n] or one index, stencil_always [n] or one flag
        (the shaded surface's material is StencilType::ALWAYS).  flavour: a name from SHADOW_FLAVOURS; `final` (flavour "regen" only):
        [n] flags, the rays of a path's last vertex.  Returns uint8 [n], 1 = the light is visible."""
        if flavour not in self.SHADOW_FLAVOURS:
            raise ValueError("unknown shadow flavour %r" % (flavour,))
        o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
        n = len(o)
        q = np.zeros(n, L.SHADOW_QUERY)
        q["org"] = o
        q["dir"] = np.ascontiguousarray(directions, np.float32).reshape(n, 3)
        q["dist_to_light"] = np.broadcast_to(np.asarray(dist_to_light, np.float32), (n,))
        q["light"] = np.broadcast_to(np.asarray(light, np.int32), (n,))
        flags = np.broadcast_to(np.asarray(stencil_always, bool), (n,)).astype(np.uint32)
        if final is not None:
            flags = flags | (np.broadcast_to(np.asarray(final, bool), (n,)).astype(np.uint32) << 1)
        q["flags"] = flags
        out = np.zeros(n, np.uint8)
        self._check(self._l.atn_trace_shadow(self._ctx, q.ctypes.data, n, self.SHADOW_FLAVOURS[flavour], out.ctypes.data))
        return out

    def shade_stage(self, records, width, height, bounce, max_depth, rr_depth, frame=0, sample=0, flavour="plain", chunk_items=0,
                    queue_order="shuffled"):
        """PathTracing::shade / ShadeMiss for n caller-given vertices (layout.SHADE_VERTEX) through ONE launch of the production shade
        kernel (atn_shade_stage): the instantiation render() picks for the uploaded scene, at this context's wave setting.  Returns
        layout.SHADE_RESULT [n]: what the next stages can observe -- flags, contrib, membership in the next queue and the shadow queue as
        the kernel appended them, the next ray / pdf / throughput / dimension of a path that goes on, the shadow record of a path that
        has one; everything else zero.  chunk_items 0 = the launch plan's, 1..4 forced; queue_order 'shuffled' or 'given'."""
        rec = np.ascontiguousarray(records, L.SHADE_VERTEX)
        call = L.shade_call(width, height, bounce, max_depth, rr_depth, frame, sample, flavour, chunk_items, queue_order)
        out = np.zeros(len(rec), L.SHADE_RESULT)
        self._check(self._l.atn_shade_stage(self._ctx, call.ctypes.data, rec.ctypes.data, len(rec), out.ctypes.data))
        return out

    def cmj_samples(self, index, dimension, scramble, n):
        out = np.zeros(n, np.float32)
        self._check(self._l.atn_cmj_samples(self._ctx, index, dimension, scramble, n, out.ctypes.data))
        return out

    def cmj_batch(self, index, dimension, scramble, draws=1):
        index = np.ascontiguousarray(index, np.uint32); dimension = np.ascontiguousarray(dimension, np.uint32)
        scramble = np.ascontiguousarray(scramble, np.uint32)
        if not (len(index) == len(dimension) == len(scramble)):
            raise ValueError("index, dimension and scramble must have one entry per triple")
        out = np.zeros((len(index), draws), np.float32)
        self._check(self._l.atn_cmj_batch(self._ctx, len(index), index.ctypes.data, dimension.ctypes.data,
                                          scramble.ctypes.data, draws, out.ctypes.data))
        return out

    LIBM_KINDS = ["sinf", "cosf", "atanf", "acosf", "atan2f", "logf", "expf", "powf", "sqrtf", "div", "inversesqrt"]

    def libm_probe(self, kind, a, b=None):
        """The device build's math library on arrays (atn_libm_probe; kind: a name from LIBM_KINDS)."""
        a = np.ascontiguousarray(a, np.float32)
        b = np.ones_like(a) if b is None else np.ascontiguousarray(b, np.float32)
        out = np.zeros_like(a)
        self._check(self._l.atn_libm_probe(self._ctx, self.LIBM_KINDS.index(kind), len(a), a.ctypes.data, b.ctypes.data, out.ctypes.data))
        return out

    def ray_offset(self, origins, normals):
        o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3); n = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        out = np.zeros_like(o)
        self._check(self._l.atn_ray_offset(self._ctx, len(o), o.ctypes.data, n.ctypes.data, out.ctypes.data))
        return out

    def material_table(self, mtrl_id, nrm, wi, index, scramble, uv, dimension=None):
        n = len(nrm)
        dim = np.ascontiguousarray(np.broadcast_to(np.asarray(dimension, np.uint32), (n,))) if dimension is not None else None
        nrm = np.ascontiguousarray(nrm, np.float32); wi = np.ascontiguousarray(wi, np.float32)
        index = np.ascontiguousarray(index, np.uint32); scramble = np.ascontiguousarray(scramble, np.uint32)
        uv = np.ascontiguousarray(uv, np.float32)
        s = np.zeros((n, 7), np.float32); e = np.zeros((n, 5), np.float32)
        self._check(self._l.atn_material_table(self._ctx, mtrl_id, n, nrm.ctypes.data, wi.ctypes.data,
                                               index.ctypes.data, dim.ctypes.data if dim is not None else None, scramble.ctypes.data, uv.ctypes.data,
                                               s.ctypes.data, e.ctypes.data))
        return s, e

    def material_eval(self, mtrl_id, nrm, wi, wo, uv=None):
        """samplePDF / sampleBSDF at given outgoing directions -> [n, 5] {pdf, bsdf.xyz, bsdf's own pdf}."""
        n = len(wo)
        b = lambda a, k: np.ascontiguousarray(np.broadcast_to(np.asarray(a, np.float32), (n, k)))
        nrm, wi, wo = b(nrm, 3), b(wi, 3), b(wo, 3)
        uv = b(uv if uv is not None else (0.5, 0.5), 2)
        e = np.zeros((n, 5), np.float32)
        self._check(self._l.atn_material_eval(self._ctx, mtrl_id, n, nrm.ctypes.data, wi.ctypes.data, wo.ctypes.data, uv.ctypes.data, e.ctypes.data))
        return e

    def compact(self, flags):
        flags = np.ascontiguousarray(flags, np.int32)
        out = np.zeros(max(1, len(flags)), np.int32)
        cnt = C.c_uint32()
        self._check(self._l.atn_compact(self._ctx, flags.ctypes.data, len(flags), out.ctypes.data, C.byref(cnt)))
        return out[:cnt.value]

    def compact2(self, flags_a, flags_b=None, grid_blocks=0):
        """The renderer's two-queue block append over caller flags; returns the queues in device order."""
        fa = np.ascontiguousarray(flags_a, np.int32)
        fb = np.ascontiguousarray(flags_b, np.int32) if flags_b is not None else None
        n = len(fa)
        oa = np.zeros(max(1, n), np.int32); ob = np.zeros(max(1, n), np.int32)
        ca = C.c_uint32(); cb = C.c_uint32()
        self._check(self._l.atn_compact2(self._ctx, fa.ctypes.data, fb.ctypes.data if fb is not None else None, n, grid_blocks,
                                         oa.ctypes.data, C.byref(ca), ob.ctypes.data if fb is not None else None,
                                         C.byref(cb) if fb is not None else None))
        return oa[:ca.value], (ob[:cb.value] if fb is not None else None)


class MultiGpuPathTracing:
    """The node-wide renderer (atn_mgpu_*, include/aten_amd.h): same calls as PathTracing, every visible GPU
    (or the given shard list; an ordinal may repeat) behind them."""

    def __init__(self, devices=None):
        self._l = lib()
        self._mg = C.c_void_p()
        if devices is None:
            rc = self._l.atn_mgpu_create(C.byref(self._mg), None, 0)
        elif isinstance(devices, int):
            rc = self._l.atn_mgpu_create(C.byref(self._mg), None, devices)
        else:
            arr = (C.c_int32 * len(devices))(*devices)
            rc = self._l.atn_mgpu_create(C.byref(self._mg), arr, len(devices))
        if rc != 0:
            raise AtenAmdError("atn_mgpu_create failed (%d)" % rc)
        self.width = self.height = 0

    def close(self):
        if self._mg:
            self._l.atn_mgpu_destroy(self._mg)
            self._mg = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise AtenAmdError("%s (status %d)" % (self._l.atn_mgpu_last_error(self._mg).decode(), rc))

    def shard_count(self):
        return int(self._l.atn_mgpu_shard_count(self._mg))

    def shard_devices(self):
        return [int(self._l.atn_mgpu_shard_device(self._mg, i)) for i in range(self.shard_count())]

    def UpdateSceneData(self, scene):
        self._check(self._l.atn_mgpu_upload_scene(self._mg, C.cast(scene.ref(), C.c_void_p)))

    def updateBVH(self, scene):
        a = scene.arrays
        objs = np.ascontiguousarray(a["objects"]); mtx = np.ascontiguousarray(a["matrices"]); top = np.ascontiguousarray(a["bvh_lists"][0])
        self._check(self._l.atn_mgpu_update_tlas(self._mg, objs.ctypes.data, len(objs), mtx.ctypes.data if len(mtx) else None,
                                                 len(mtx), top.ctypes.data, len(top)))

    # ---- scene edits (docs/SCENE_EDITS.md; idaten::Renderer::updateMaterial / updateLight / UpdateTexture /
    # UpdateSceneRenderingConfig, renderer.cpp:207-252): each reads the edited data from `scene` (a SceneBuilder result, or
    # anything with its `desc`), whose counts and texture sizes are the uploaded ones.  Nothing is reset: call reset() for that.
    def updateMaterial(self, scene, first=0, n=None):
        """Materials [first, first + n) of `scene` (default: from `first` to the end) replace the uploaded ones."""
        d = scene.desc
        n = int(d.n_materials) - first if n is None else n
        self._check(self._l.atn_mgpu_update_materials(self._mg, _elem_ptr(d.materials, first, L.MATERIAL_PARAM), n, first))

    def updateLight(self, scene, npr_target=False, first=0, n=None):
        """Lights [first, first + n) of `scene`; npr_target: of its NPR target lights."""
        d = scene.desc
        base, count = (d.npr_target_lights, d.n_npr_target_lights) if npr_target else (d.lights, d.n_lights)
        n = int(count) - first if n is None else n
        self._check(self._l.atn_mgpu_update_lights(self._mg, _elem_ptr(base, first, L.LIGHT_PARAM), n, first, 1 if npr_target else 0))

    def UpdateTexture(self, scene, texid):
        """Texture `texid` of `scene` (same size as uploaded) replaces the uploaded one."""
        d = scene.desc
        if texid < 0 or texid >= int(d.n_textures):
            raise ValueError("UpdateTexture: the scene has no texture %d" % texid)
        tex = C.cast(d.textures, C.POINTER(L.TextureDesc))
        self._check(self._l.atn_mgpu_update_texture(self._mg, texid, C.byref(tex[texid])))

    def UpdateSceneRenderingConfig(self, scene):
        """The rendering config of `scene` (atn_scene_desc::config) replaces the uploaded one."""
        self._check(self._l.atn_mgpu_update_rendering_config(self._mg, C.byref(scene.desc.config)))

    # ---- dynamic geometry (the reference's deformation renderer, src/deformation_renderer/main.cpp:636-710)
    def updateGeometry(self, vtx_pos=None, vtx_nml=None, vtx_offset=0, triangles=None, tri_offset=0):
        """idaten::Renderer::updateGeometry (renderer.cpp:155-215): overwrite a vertex / triangle range of the scene."""
        from . import layout as L
        pos = None if vtx_pos is None else np.ascontiguousarray(vtx_pos, np.float32).reshape(-1, 4)
        nml = None if vtx_nml is None else np.ascontiguousarray(vtx_nml, np.float32).reshape(-1, 4)
        if pos is not None and nml is not None and len(pos) != len(nml):
            raise ValueError("updateGeometry: %d positions but %d normals (the C ABI takes ONE vertex count for both arrays)" % (len(pos), len(nml)))
        nv = len(pos) if pos is not None else (len(nml) if nml is not None else 0)
        tr = None if triangles is None else np.ascontiguousarray(triangles, L.TRIANGLE_PARAM)
        self._check(self._l.atn_mgpu_update_geometry(self._mg, pos.ctypes.data if pos is not None else None, nml.ctypes.data if nml is not None else None,
                               nv, vtx_offset, tr.ctypes.data if tr is not None else None, len(tr) if tr is not None else 0, tri_offset))

    def lbvh_rebuild_list(self, list_index, tri_offset, n_triangles, bbox_min, bbox_max):
        """idaten::LBVHBuilder::build into the renderer's node list (LBVHBuilder.cu:700-810), on the device."""
        f3 = lambda v: (C.c_float * 3)(*[float(x) for x in v])
        self._check(self._l.atn_mgpu_lbvh_rebuild_list(self._mg, list_index, tri_offset, n_triangles, f3(bbox_min), f3(bbox_max)))

    def tlas_rebuild(self, objects=None, matrices=None, force_general=False):
        """PathTracing.tlas_rebuild on every shard."""
        objs = None if objects is None else np.ascontiguousarray(objects, L.OBJECT_PARAM)
        mtx = None if matrices is None else np.ascontiguousarray(matrices, np.float32).reshape(-1, 4, 4)
        self._check(self._l.atn_mgpu_tlas_rebuild(self._mg, objs.ctypes.data if objs is not None else None, len(objs) if objs is not None else 0,
                                                  mtx.ctypes.data if mtx is not None and len(mtx) else None, len(mtx) if mtx is not None else 0,
                                                  1 if force_general else 0))

    def updateCamera(self, cam):
        self._check(self._l.atn_mgpu_update_camera(self._mg, cam.ctypes.data))

    def initSampler(self, width, height, seed=0):
        self._check(self._l.atn_mgpu_init_sampler(self._mg, width, height, seed))

    def render(self, width, height, max_depth=5, rr_depth=3, spp=1, frame=0, progressive=True,
               break_on_terminate=True, download=True):
        d = Destination(width, height, max_depth, rr_depth, spp, frame, int(progressive), int(break_on_terminate), 0, 0)
        out = np.empty((height, width, 4), np.float32) if download else None
        self._check(self._l.atn_mgpu_render(self._mg, C.byref(d), out.ctypes.data if download else None))
        self.width, self.height = width, height
        return out

    def set_regeneration(self, on):
        self._check(self._l.atn_mgpu_set_regeneration(self._mg, int(on)))

    def set_sphere_intersection(self, mode):
        """PathTracing.set_sphere_intersection on every shard (read by the next upload)."""
        self._check(self._l.atn_mgpu_set_sphere_intersection(self._mg, int(mode)))

    def render_burst(self, width, height, n_frames, max_depth=5, rr_depth=3, spp=1, frame=0, progressive=True,
                     break_on_terminate=True, download=True):
        """n_frames consecutive frames on every shard, one exchange of the tiles at the end."""
        d = Destination(width, height, max_depth, rr_depth, spp, frame, int(progressive), int(break_on_terminate), 0, 0)
        out = np.empty((height, width, 4), np.float32) if download else None
        self._check(self._l.atn_mgpu_render_burst(self._mg, C.byref(d), n_frames, out.ctypes.data if download else None))
        self.width, self.height = width, height
        return out

    def reset(self):
        self._check(self._l.atn_mgpu_reset(self._mg))

    def synchronize(self):
        self._check(self._l.atn_mgpu_synchronize(self._mg))

    def set_frames_in_flight(self, n):
        self._check(self._l.atn_mgpu_set_frames_in_flight(self._mg, n))

    def film_device_ptr(self):
        return self._l.atn_mgpu_film_device(self._mg)

    def download_film(self):
        out = np.empty((self.height, self.width, 4), np.float32)
        self._check(self._l.atn_mgpu_download_film(self._mg, out.ctypes.data))
        return out

    # ---- node-wide SVGF (docs/MGPU_SVGF.md): the path pass on every shard, the hand-over planes gathered to shard 0, the filters there
    SVGF_BUFFERS = PathTracing.SVGF_BUFFERS

    def svgf_render(self, width, height, max_depth=5, rr_depth=3, spp=1, frame=0, compute_motion=False, stages=False,
                    download=True, profile=False):
        """PathTracing.svgf_render for the whole node: the filtered frame [h, w, 4] (and the three intermediate puts), byte-equal to
        one context's whatever the shard count.  After a failure call svgf_reset() before the next frame."""
        d = Destination(width, height, max_depth, rr_depth, spp, frame, 0, 1, 0, int(profile))
        out = np.empty((height, width, 4), np.float32) if download else None
        st = np.empty((3, height, width, 4), np.float32) if stages else None
        self._check(self._l.atn_mgpu_svgf_render(self._mg, C.byref(d), int(compute_motion),
                                                 out.ctypes.data if download else None, st.ctypes.data if stages else None))
        self.width, self.height = width, height
        return (out, st) if stages else out

    def svgf_set_motion_depth(self, md):
        md = np.ascontiguousarray(md, np.float32).reshape(-1, 4)
        self._check(self._l.atn_mgpu_svgf_set_motion_depth(self._mg, md.ctypes.data, len(md)))

    def svgf_reset(self):
        self._check(self._l.atn_mgpu_svgf_reset(self._mg))

    def svgf_set_dilate_temporal_weight(self, on):
        self._check(self._l.atn_mgpu_svgf_set_dilate_temporal_weight(self._mg, int(on)))

    def svgf_set_atrous_iterations(self, n):
        self._check(self._l.atn_mgpu_svgf_set_atrous_iterations(self._mg, n))

    def svgf_buffer(self, name):
        """A buffer of the last node-wide SVGF frame (shard 0's planes), float32 [h, w, 4]; names as PathTracing.svgf_buffer."""
        out = np.empty((self.height, self.width, 4), np.float32)
        self._check(self._l.atn_mgpu_svgf_download(self._mg, self.SVGF_BUFFERS[name], out.ctypes.data))
        return out

    def svgf_output_device_ptr(self):
        return self._l.atn_mgpu_svgf_output_device(self._mg)

    def kernel_times(self, shard=0):
        """HIP-event time and launch count per kernel class of one shard's profiled frames (MGPU_K_NAMES: 'svgf_pack' on shards
        1 .. N-1, 'svgf_unpack' on shard 0)."""
        ms = np.zeros(len(MGPU_K_NAMES), np.float32); n = np.zeros(len(MGPU_K_NAMES), np.uint32)
        self._check(self._l.atn_mgpu_get_kernel_times(self._mg, shard, ms.ctypes.data, n.ctypes.data))
        return {k: (float(ms[i]), int(n[i])) for i, k in enumerate(MGPU_K_NAMES)}

    def reset_kernel_times(self):
        self._check(self._l.atn_mgpu_reset_kernel_times(self._mg))


class VolumeGrid(C.Structure):
    """atn_volume_grid (include/aten_amd.h)."""
    _fields_ = [("dim", C.c_int32 * 3), ("origin", C.c_float * 3), ("voxel_size", C.c_float), ("density", C.c_void_p)]


VOLUME_STATE_FLAGS = dict(processed=1, hit=2, sampled=4, absorbed=8, scattered=16, passed=32, connection=64, terminated=256)


def unpack_primary_hit(plane):
    """The ids plane ('primary_hit') as dict(objid int32 [h, w] (-1 = miss), tri int32 [h, w], a, b float32 [h, w])."""
    p = np.ascontiguousarray(plane, np.float32)
    return dict(objid=p[..., 0].copy().view(np.int32), tri=p[..., 1].copy().view(np.int32), a=p[..., 2].copy(), b=p[..., 3].copy())


def unpack_volume_state(raw):
    """uint32 [h, w, 4] {flags, depth_count, stack size, CMJ dimension} of atn_volume_download(0) -> dict."""
    out = {k: (raw[..., 0] & v) != 0 for k, v in VOLUME_STATE_FLAGS.items()}
    out.update(depth_count=raw[..., 1].astype(np.int32), stack_size=raw[..., 2].astype(np.int32), dim=raw[..., 3].copy(),
               flight_steps=((raw[..., 0] >> 16) & 0x7fff).astype(np.int32))
    return out


def unpack_volume_stack(raw, size):
    """uint32 [h, w, 4] (eight 16-bit ids, the newest in the low half of word 0) + the stack size -> int32 [h, w, 8] in the order the
    media were entered, zeros beyond the size."""
    half = np.stack([(raw[..., k // 2] >> (16 * (k % 2))) & 0xffff for k in range(8)], axis=-1).astype(np.int32)      # newest first
    size = np.asarray(size, np.int64)
    k = np.arange(8)
    src = size[..., None] - 1 - k
    out = np.take_along_axis(half, np.clip(src, 0, 7), axis=-1)
    return np.where(src >= 0, out, 0).astype(np.int32)
