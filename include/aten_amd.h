/*
 * aten_amd.h -- C-ABI of the MI355X path-tracing integrator (libaten_amd.so).
 *
 * Drop-in boundary: these entry points take exactly the flat arrays that aten's existing GPU
 * seam, idaten::Renderer (src/libidaten/kernel/renderer.h:17-179 of the reference), extracts
 * from aten::context, and perform what idaten::PathTracing does with them -- but with the
 * sample stream and semantics of the CPU renderer aten::PathTracing (the parity target).
 * INTEGRATION.md shows the C++ adapter an aten application adds.
 *
 * All functions return 0 on success or a negative atn_status; they never throw.  A context is
 * not thread-safe (the reference's renderer objects are single-threaded, one per window thread);
 * distinct contexts are independent.  The library fails loudly (ATN_ERR_NO_DEVICE) when no HIP
 * device is present: there is no CPU fallback.
 */
#ifndef ATEN_AMD_H_
#define ATEN_AMD_H_

#include "aten_layout.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct atn_ctx atn_ctx;

typedef enum atn_status {
    ATN_OK = 0,
    ATN_ERR_INVALID_ARG = -1,
    ATN_ERR_NO_DEVICE = -2,
    ATN_ERR_HIP = -3,
    ATN_ERR_NO_SCENE = -4,
    ATN_ERR_UNSUPPORTED = -5,
    ATN_ERR_OUT_OF_MEMORY = -6
} atn_status;

/* aten::Destination (src/libaten/renderer/renderer.h:15-23) plus what the reference keeps as
 * renderer state: the frame counter (renderer.h:31-39,71; CPU starts at 0, CUDA at 1) and the
 * film flavour (Film vs FilmProgressive, src/libaten/renderer/film.cpp:33-71). */
typedef struct atn_destination {
    int32_t width;
    int32_t height;
    int32_t maxDepth;
    int32_t russianRouletteDepth;
    int32_t sample;                 /* samples per pixel this frame */
    uint32_t frame;                 /* aten::Renderer::GetFrameCount() */
    int32_t progressive;            /* 1 = FilmProgressive::put running mean, 0 = Film::put overwrite */
    int32_t break_on_terminate;     /* 1 = reproduce pathtracing.cpp:350-352 (stop sampling a pixel after a
                                       terminated path; the CPU renderer's behaviour), 0 = take all samples */
    int32_t count_stats;            /* 1 = count rays / node visits / triangle tests (slower; atn_get_stats) */
    int32_t profile;                /* 1 = bracket every launch with HIP events (atn_get_kernel_times) */
} atn_destination;

/* ≙ idaten::Renderer construction + cudaSetDevice.  device_ordinal: HIP device index. */
int atn_create(atn_ctx** out, int device_ordinal);
void atn_destroy(atn_ctx* ctx);
const char* atn_last_error(atn_ctx* ctx);

/* ≙ idaten::Renderer::UpdateSceneData (src/libidaten/kernel/renderer.cpp:12-131): copies the
 * scene to HBM (and re-lays-out the BVH).  The caller keeps ownership of `scene`.
 * ATN_ERR_UNSUPPORTED for an id out of range: an object, matrix, triangle, vertex, material or light id, and a texture index
 * (a material's maps, an IBL light's envmapidx, the config's envmap_tex_idx; negative = none) that is not below n_textures. */
int atn_upload_scene(atn_ctx* ctx, const atn_scene_desc* scene);

/* ≙ idaten::Renderer::updateBVH (src/libidaten/kernel/renderer.cpp:133-153): new ObjectParameters and
 * matrices (aten::context::GetObjectParametersAndMatrices) and a rebuilt TOP layer (`nodes[0]`); the
 * bottom-level lists uploaded by atn_upload_scene stay in place.  n_matrices == 0 keeps the old
 * matrices, like the reference.  The list indices in the leaves' exid refer to the uploaded lists. */
int atn_update_tlas(atn_ctx* ctx, const atn_object_param* objects, uint32_t n_objects,
                    const atn_mat4* matrices, uint32_t n_matrices,
                    const atn_bvh_node* top_nodes, uint32_t n_top_nodes);

/* How atn_upload_scene lays the scene out.  Context state, initialised ONCE at atn_create from the environment variables of the same
 * names (README.md) and changed only here -- not re-read from the process environment at every upload.  -1 leaves an option as it is.
 *   anyhit_twin       0 / 1 / 2: no any-hit twins / where the surface-area model expects them to pay (default) / wherever possible
 *   anyhit_twin_dirs  8 / 1: one twin per octant of the ray direction (default) / the one direction-free twin
 *   node_layout       1 / 0: first levels of a list level by level (default) / walk order
 *   planar_lights     1 / 0: shadow rays towards planar, rigidly placed area lights stop at the first nearer hit (default) / never
 * Films do not depend on any of them (tests/test_gpu_anyhit_twin.py). */
int atn_set_upload_options(atn_ctx* ctx, int32_t anyhit_twin, int32_t anyhit_twin_dirs, int32_t node_layout, int32_t planar_lights);

/* Analytic spheres in the walk (docs/SPHERES.md).  Context state with the lifetime of the upload options above: read by the next
 * atn_upload_scene / atn_update_tlas.
 *   mode 0 (default)  a top-layer leaf of an ATN_OBJ_SPHERE object is never tested, as in aten::ThreadedBvhTraverser: the sphere can
 *                     be sampled as a light and is invisible to every ray
 *   mode 1            such leaves are tested with sphere::hit by every ray of atn_render, atn_trace_closest and atn_trace_shadow; a leaf
 *                     without triangle and nested tree that is anything else refuses the upload (ATN_ERR_UNSUPPORTED)
 * atn_sphere_leaves: how many leaves of the uploaded scene are tested (0 in mode 0).  While it is above 0 the other renderers, path
 * regeneration and bursts, relaxed shade math, deferred NEE, atn_tlas_rebuild, atn_shade_stage and geometry motion are refused. */
int atn_set_sphere_intersection(atn_ctx* ctx, int32_t mode);
int atn_sphere_leaves(atn_ctx* ctx, uint32_t* n);

/* ≙ idaten::Renderer::updateCamera (renderer.cpp:202-205). */
int atn_update_camera(atn_ctx* ctx, const atn_camera_param* camera);

/* ---- scene edits (docs/SCENE_EDITS.md): ≙ idaten::Renderer::updateMaterial / updateLight / UpdateTexture /
 * UpdateSceneRenderingConfig (renderer.cpp:207-252).  `first` and `n` name a range of the uploaded array (the reference's call
 * is first = 0); counts never change.  npr_target != 0 addresses atn_scene_desc::npr_target_lights instead of lights.  A
 * texture update keeps the texture's width and height.
 * After a successful edit the context behaves as one that was handed the edited atn_scene_desc by atn_upload_scene -- every
 * film of every renderer, every refusal, atn_rr_lookahead_active, atn_nee_deferral_active and atn_sample_texture -- except that
 * what was made on the device since the upload survives (skins, rebuilt lists, the geometry-motion history, films and the
 * renderers' histories) and that atn_planar_area_lights may be lower: a light whose type and arealight_objid are unchanged keeps
 * its planar flag, any other edited light loses it, no edit grants one (films do not depend on the flag).
 * The calls wait for the frames in flight, reset nothing (atn_reset where the reference's reset() is wanted) and are atomic: a
 * refused edit changes nothing.  ATN_ERR_NO_SCENE before an upload; ATN_ERR_INVALID_ARG for null pointers and ranges outside
 * the uploaded counts; ATN_ERR_UNSUPPORTED, with atn_upload_scene's message, for content the upload refuses (a texture, object
 * or NPR target light index out of range) and for a texture of another size.  Additive entry points: atn_abi_version stays 3. */
int atn_update_materials(atn_ctx* ctx, const atn_material_param* materials, uint32_t n, uint32_t first);
int atn_update_lights(atn_ctx* ctx, const atn_light_param* lights, uint32_t n, uint32_t first, int32_t npr_target);
int atn_update_texture(atn_ctx* ctx, int32_t texid, const atn_texture_desc* tex);
int atn_update_rendering_config(atn_ctx* ctx, const atn_scene_rendering_config* config);

/* Scene updates between frames -- atn_update_tlas, atn_update_geometry, atn_lbvh_rebuild_list -- return when they are
 * ENQUEUED: the caller's arrays have been copied (they may be reused at once), the frames in flight keep running, and
 * every frame rendered afterwards sees the update.  With atn_set_frames_in_flight > 1 the mutable part of the scene is
 * kept once per frame in flight (up to three copies) on the device for this. */

/* ---- dynamic geometry: the per-tick sequence of the reference's deformation renderer
 * (src/deformation_renderer/main.cpp:636-710): skinned vertices -> LBVHBuilder::build into the renderer's node list ->
 * Renderer::updateGeometry -> Renderer::updateBVH (= atn_update_tlas). */

/* ≙ idaten::Renderer::updateGeometry (src/libidaten/kernel/renderer.cpp:155-215): overwrite vertices
 * [vtx_offset, vtx_offset + n_vertices) and triangles [tri_offset, tri_offset + n_triangles) of the uploaded scene.  Host
 * pointers; vtx_pos or vtx_nml may be NULL (left as they are).  Bottom-level lists over these triangles must be rebuilt
 * (atn_lbvh_rebuild_list) before the next render: their leaf records hold vertex data. */
int atn_update_geometry(atn_ctx* ctx, const atn_vec4* vtx_pos, const atn_vec4* vtx_nml, uint32_t n_vertices, uint32_t vtx_offset,
                        const atn_triangle_param* triangles, uint32_t n_triangles, uint32_t tri_offset);
/* The scene arrays in device memory (float4[n_vertices] x 2, atn_triangle_param[n_triangles]) for a caller whose own HIP
 * skinning kernel writes them in place (≙ the interop VBO the reference's skinning writes, main.cpp:673-676).  Waits for
 * the frames in flight and switches the context to ONE copy of the scene, updated in place behind the frames in flight
 * (the caller's kernel must itself run after them, e.g. after atn_synchronize); the pointers stay valid until the next
 * atn_upload_scene. */
int atn_scene_device_arrays(atn_ctx* ctx, void** vtx_pos, void** vtx_nml, void** triangles);
/* ≙ lbvh_.build(nodes[deformPos], tris, tri_offset_, sceneBbox, vtxPos, ...) (main.cpp:686-693; idaten::LBVHBuilder::onBuild,
 * src/libidaten/kernel/LBVHBuilder.cu:700-810): rebuild bottom-level list `list_index` ON THE DEVICE as an LBVH over the
 * scene's triangles [tri_offset, tri_offset + n_triangles) as they are in device memory now; bbox_* is the box the Morton
 * codes are normalised with (the reference passes the skinned mesh's box).  The tree is the reference's, node for node;
 * its records replace the list's region of the node image, which must hold exactly n - 1 inner and n leaf records (a list
 * uploaded as a binary tree with one leaf per triangle).  ATN_ERR_UNSUPPORTED otherwise. */
int atn_lbvh_rebuild_list(atn_ctx* ctx, uint32_t list_index, uint32_t tri_offset, uint32_t n_triangles,
                          const float bbox_min[3], const float bbox_max[3]);
/* ≙ idaten::LBVHBuilder::build(dst, std::vector<TriangleParameter>&, triIdOffset, sceneBbox, vtxPos, vtxOffset,
 * threadedBvhNodes) (LBVHBuilder.cu:812-833): the same builder as a function of host arrays, returning
 * ThreadedBvhNode[2 n - 1] in the reference's node order (inner nodes 0 .. n-2, leaves n-1 .. 2n-2; leaf f0 = 1,
 * f1 = tri_id_offset + triangle index).  out_sorted_codes / out_sorted_indices (n each) may be NULL.  Needs no scene. */
int atn_lbvh_build(atn_ctx* ctx, const atn_triangle_param* triangles, uint32_t n_triangles, int32_t tri_id_offset,
                   const float bbox_min[3], const float bbox_max[3], const atn_vec4* vtx_pos, uint32_t n_vertices, int32_t vtx_offset,
                   atn_bvh_node* out_nodes, uint32_t* out_sorted_codes, uint32_t* out_sorted_indices);

/* ---- skinning on the device: the first step of that sequence (idaten::Skinning, src/libidaten/kernel/Skinning.cu; docs/SKINNING.md).
 * A tick uploads one matrix per bone; the skinned vertices, the triangles' areas, the shading records and the mesh's box are
 * computed in device memory behind the frames in flight.  A skin is named by a handle (never 0); it dies with atn_skin_destroy
 * and with every atn_upload_scene, and every call on a dead handle returns ATN_ERR_INVALID_ARG.  Refused (ATN_ERR_UNSUPPORTED):
 * a context whose scene arrays the caller writes itself (atn_scene_device_arrays).  There is no atn_mgpu_* form.
 * Additive entry points: atn_abi_version stays 3. */
typedef uint32_t atn_skin;
/* ≙ Skinning::initWithTriangles + setVtxOffset: binds `vertices` to vertices [vtx_offset, vtx_offset + n_vertices) and triangles
 * [tri_offset, tri_offset + n_triangles) of the uploaded scene (n_triangles may be 0).  The scene's triangles hold final vertex
 * indices: there is no index offset to maintain.  Checked here, once, on the host -- nothing out of range reaches a kernel:
 * ATN_ERR_INVALID_ARG for a range outside the scene or a triangle of the range naming a vertex outside the skin's vertices,
 * ATN_ERR_UNSUPPORTED for an (int)blend_index outside [0, n_matrices) (also under a weight of 0: all four matrices are read) or
 * n_matrices > 65536.  Waits for the frames in flight. */
int atn_skin_create(atn_ctx* ctx, const atn_skinning_vertex* vertices, uint32_t n_vertices, uint32_t vtx_offset,
                    uint32_t tri_offset, uint32_t n_triangles, uint32_t n_matrices, atn_skin* out_skin);
/* ≙ Skinning::update: the palette for the next atn_skin_compute; n must be the skin's n_matrices.  Enqueued; `matrices` is free on return. */
int atn_skin_update(atn_ctx* ctx, atn_skin skin, const atn_mat4* matrices, uint32_t n);
/* ≙ Skinning::compute, enqueued behind the frames in flight: writes the skin's range of the scene's vertex positions (w = uv[0]) and
 * normals (w = uv[1]), the triangles' areas (|cross|, not halved) and shading records, keeps the previous positions (is_restart: the
 * new ones; otherwise the positions before this call, w = 1) and leaves the mesh's box in device memory.  With bbox_min and bbox_max
 * it then waits and returns the box (the reference's read-back); with both NULL it returns at once.  ATN_ERR_INVALID_ARG before the
 * first atn_skin_update.  Bottom-level lists over the triangles must be rebuilt before the next render. */
int atn_skin_compute(atn_ctx* ctx, atn_skin skin, int32_t is_restart, float bbox_min[3], float bbox_max[3]);
/* atn_lbvh_rebuild_list over the skin's triangles with the Morton codes normalised by the skin's box AS IT IS IN DEVICE MEMORY (after
 * atn_skin_compute): no read-back.  Same tree, same refusals. */
int atn_lbvh_rebuild_list_skinned(atn_ctx* ctx, uint32_t list_index, atn_skin skin);
/* Rebuild the TOP layer on the device as an LBVH over the instances' world boxes (docs/TLAS.md), enqueued behind the frames in flight
 * like atn_update_tlas: no host tree, no host wait, nothing read back.  An instance's local box is the root record of its list as it
 * is in device memory at that point of the update stream -- after atn_lbvh_rebuild_list[_skinned] the new LBVH's root, so a skinned
 * tick needs neither a box read-back nor a conservative box.
 * objects / matrices: as atn_update_tlas; NULL objects (n_objects == 0) keeps the uploaded ones, n_matrices == 0 keeps the old matrices.
 * flags bit 0: force the general (multi-launch) path; both paths write the same bytes.
 * The set of leaves is the last host-given top layer's (atn_upload_scene, atn_update_tlas): objid, the list it enters, meshid.  Leaves
 * with neither triangles nor a nested tree (sphere instances, never tested by the walk) are dropped from a rebuilt layer.  Binding an
 * instance to another list, or another number of instances, still needs atn_update_tlas.
 * ATN_ERR_NO_SCENE before an upload; ATN_ERR_INVALID_ARG for a null array with a count (or a count without an array);
 * ATN_ERR_UNSUPPORTED for ids out of range, more than 2^23 instances, and a top layer without an instance leaf.  A refused call
 * changes nothing.  Additive entry points: atn_abi_version stays 3. */
int atn_tlas_rebuild(atn_ctx* ctx, const atn_object_param* objects, uint32_t n_objects,
                     const atn_mat4* matrices, uint32_t n_matrices, uint32_t flags);
/* Probe: the top-layer records of the current scene set as they are in device memory (32-byte records, the root first; DESIGN.md
 * "data layout in HBM").  Waits for everything.  out may be NULL (the counts only); cap_bytes is the size of `out`. */
int atn_tlas_download(atn_ctx* ctx, void* out, uint32_t cap_bytes, uint32_t* out_records, int32_t* out_root_link, uint32_t* out_top_base);
/* For tests; waits for everything.  which = 0 positions, 1 normals, 2 previous positions (atn_vec4[n_vertices]), 3 the box
 * (float[6]: min, max), 4 the triangles' areas (float[n_triangles]); and of the WHOLE scene as new frames read it: 5 the shading
 * records (8 atn_vec4 per triangle), 6 positions, 7 normals (atn_vec4 per vertex), 8 triangles (atn_triangle_param). */
int atn_skin_download(atn_ctx* ctx, atn_skin skin, int32_t which, void* out_host);
/* For tests; waits for everything.  The bytes of bottom-level list `list_index` in the node image, any-hit twins included;
 * out_host may be NULL (size only). */
int atn_skin_download_list(atn_ctx* ctx, uint32_t list_index, void* out_host, uint32_t capacity_bytes, uint32_t* n_bytes);
int atn_skin_destroy(atn_ctx* ctx, atn_skin skin);

/* ≙ aten::initSampler(width, height, seed) (src/libaten/sampler/sampler.cpp:8-18) followed by
 * idaten::PathTracing::initSamplerParameter's upload of aten::getRandom()
 * (src/libidaten/kernel/renderer.h:113-124): one std::mt19937(seed) draw per pixel. */
int atn_init_sampler(atn_ctx* ctx, int32_t width, int32_t height, int32_t seed);
/* Same, with caller-provided seeds (aten::getRandom()). */
int atn_set_random(atn_ctx* ctx, const uint32_t* seeds, uint32_t n);
/* ≙ aten::getRandom() (src/libaten/sampler/sampler.cpp:20-23): the first n entries of the table the kernels
 * read, copied back from HBM; atn_random_count = its size (0 before atn_init_sampler / atn_set_random). */
int atn_get_random(atn_ctx* ctx, uint32_t* out_host, uint32_t n);
uint32_t atn_random_count(atn_ctx* ctx);

/* Screen-space sharding for multi-GPU: the image is cut into 8x8-pixel tiles, tile t (row-major)
 * is rendered by rank t % world.  Default (0, 1) = whole image.  No reference analogue (the
 * reference is single-GPU). */
int atn_set_screen_shard(atn_ctx* ctx, int32_t rank, int32_t world);

/* ≙ idaten::PathTracing::render(width, height, maxSamples, maxBounce)
 * (src/libidaten/kernel/pathtracing.cpp:49-153) with aten::PathTracing::OnRender's semantics
 * (src/libaten/renderer/pathtracing/pathtracing.cpp:269-366).
 * out_host: optional vec4[width*height], row 0 = bottom (like aten::Film); NULL = stay on device. */
int atn_render(atn_ctx* ctx, const atn_destination* dst, atn_vec4* out_host);

/* ---- path regeneration (BASELINE.json north_star: "path compaction/regeneration") ---------------------------------------------
 * The loop behind atn_render is the reference's (src/libidaten/kernel/pathtracing.cpp:105-138): sample by sample, bounce by bounce, one
 * compaction per bounce, on a ray population that decays until the sample's longest path is over.  With regeneration on, a frame's
 * samples -- and, through atn_render_burst, a run of consecutive progressive frames -- share one POOL of path slots, one per pixel: the
 * moment a pixel's path ends, the shade kernel runs its sample epilogue (pathtracing.cpp:339-352; after the frame's last sample
 * Film::put / FilmProgressive::put, film.cpp:33-71) and writes the pixel's next primary ray (GeneratePath, pathtracing_impl.h:65-110)
 * into the same slot, so every launch works on a full population.  Per pixel the samples and frames keep the serial order and
 * arithmetic: films are BYTE-equal to the serial loop's, with both values of break_on_terminate, on any screen shard.
 *
 * atn_set_regeneration: 0 = the serial loop (default), 1 = the pool wherever it applies: atn_render with sample > 1 and atn_render_burst
 * (not with count_stats -- counted frames use the serial loop's counting kernels -- and not atn_svgf_render, whose AOVs are per frame).
 * atn_render_burst: n_frames x atn_render with frame = dst->frame, dst->frame + 1, ... (the serial loop does exactly that when
 * regeneration is off or does not apply; n_frames > 1 regenerates only with dst->progressive); out_host receives the film after the last.
 * atn_regen_stage_counts: closest-hit rays and shadow rays of every launch of the last regenerated burst (the pool's occupancy),
 * n_stages entries (at most `capacity` written); either array may be NULL. */
int atn_set_regeneration(atn_ctx* ctx, int32_t mode);
int32_t atn_get_regeneration(atn_ctx* ctx);
int atn_render_burst(atn_ctx* ctx, const atn_destination* dst, int32_t n_frames, atn_vec4* out_host);
int atn_regen_stage_counts(atn_ctx* ctx, uint32_t* closest, uint32_t* shadow, uint32_t capacity, uint32_t* n_stages);

/* Floating-point rules of the shade kernel.  0 (default): every operation rounds as the CPU renderer's SSE2 build does -- no fused
 * multiply-add, correctly rounded division and square root, ocml's sinf / cosf / ...: the parity path, what every test and the
 * headline number use.  1: the rules of the reference's own GPU build (src/libidaten/CMakeLists.txt:188, nvcc --use_fast_math): fused
 * multiply-adds, approximate division / square root, the hardware's transcendentals, denormals flushed.  Frames then differ from the
 * CPU renderer's beyond the parity tolerance (measured: DESIGN.md section 7f); serial loop only (not the regenerated pool, not SVGF). */
int atn_set_shade_math(atn_ctx* ctx, int32_t mode);

/* The roulette look-ahead of atn_render's serial sample loop.  Where Russian roulette applies (bounce > russianRouletteDepth), whether a
 * path survives its NEXT vertex is known one bounce earlier: the probability is max3 of the throughput it arrives with and the draw a
 * pure function of the stored sampler position.  A path that will lose is traced as an any-hit ray -- a miss adds the environment as
 * ever, a hit only ends it -- and its hit is not shaded.  Films are byte-equal with and without.
 * Valid only on scenes in which no material draws in front of the roulette, skips NEE's draws or emits (no Emissive, singular,
 * translucent, CarPaint, Toon / StylizedBrdf material): decided at atn_upload_scene; atn_rr_lookahead_active tells (1 / 0) whether
 * frames of the current scene run it.  mode 0 = off; 1 (default; ATEN_AMD_RR_LOOKAHEAD at atn_create) = on, frames with count_stats = 1
 * keep the reference's accounting (off); 2 = counted frames too: atn_get_stats then counts the rays walked to their closest hit and
 * the hits that are shaded, and atn_rr_lookahead_stats the rest: {doomed rays, doomed hits (not shaded), node visits and triangle
 * tests of the doomed rays}.  Not applied by the regenerated pool, SVGF, ReSTIR, NPR, AO, volume frames or atn_set_shade_math(1). */
int atn_set_rr_lookahead(atn_ctx* ctx, int32_t mode);
int32_t atn_rr_lookahead_active(atn_ctx* ctx);
int atn_rr_lookahead_stats(atn_ctx* ctx, uint64_t out[4]);

/* The deferred NEE of atn_render's serial sample loop.  HitShadowRay adds a vertex's light sample only if its shadow ray reaches the
 * light, so in a deferred frame shade casts the ray from the sample's geometry alone and the rest of the sample -- the environment
 * texel, the second BSDF evaluation, the MIS weight -- is evaluated after the ray has been traced, for the rays that reached their
 * light: one small launch per bounce replays those vertices with shade's own functions.  Films are byte-equal in every mode
 * (docs/NEE_DEFERRAL.md).  A scene qualifies when its material set is Core, Disney or Analytic (no CarPaint, Toon / StylizedBrdf
 * material) and it has a light; decided at atn_upload_scene.  mode 0 = off: the mode a context starts in (ATEN_AMD_NEE_DEFERRAL at
 * atn_create selects another) -- measured, the headline frame does not gain (docs/NEE_DEFERRAL.md); 1 = every scene that qualifies;
 * 2 = the policy: scenes that qualify AND whose lights are all infinite (environment, directional): under an area lamp most shadow
 * rays reach the light and the replay costs more than it saves.  A bank allocates the mode's extra state (36 bytes per path slot)
 * when it first runs a deferred frame.  atn_nee_deferral_active tells (1 / 0) whether
 * frames of the current scene run it.  Frames with count_stats = 1 stay eager (the reference's ray accounting).
 * atn_nee_deferral_stats: {shadow rays cast, rays that reached the light} over the deferred frames since the last atn_reset -- a caller
 * whose scene lets most rays through can see it and switch the mode off.  ATN_K_TRACE_SHADOW times the evaluation launches.  Not
 * applied by the regenerated pool, SVGF, ReSTIR, NPR, AO, volume frames or atn_set_shade_math(1). */
int atn_set_nee_deferral(atn_ctx* ctx, int32_t mode);
int32_t atn_nee_deferral_active(atn_ctx* ctx);
int atn_nee_deferral_stats(atn_ctx* ctx, uint64_t out[2]);

/* ≙ idaten::Renderer::reset (renderer.h:40-43): clears the progressive film. */
int atn_reset(atn_ctx* ctx);

/* Device-side results of the last atn_render (valid until the next call on ctx). */
void* atn_film_device(atn_ctx* ctx);            /* float4[width*height]; only this rank's pixels are written */
void* atn_tile_device(atn_ctx* ctx);            /* float4[atn_tile_slots]: this rank's pixels in slot order */
/* How many bottom-level lists of the uploaded scene have an any-hit twin right now (csrc/host/anyhit_twin.hpp: a second threading
 * of the same tree that the shadow rays of infinite lights walk; results do not depend on it).  ATEN_AMD_ANYHIT_TWIN = 0 / 1 / 2 at
 * upload: none / where the surface-area model expects it to pay (default) / wherever a list is a binary tree.  An LBVH rebuild of a
 * list re-threads its twins on the device from the new tree. */
uint32_t atn_anyhit_twins(atn_ctx* ctx);
/* How many area lights' shadow rays may stop at the first hit nearer than the light right now: lights whose object is planar and placed
 * by a rigid matrix, found at upload (csrc/host/scene_upload.hpp, planar_area_light; ATEN_AMD_PLANAR_LIGHTS=0 switches the rule off).
 * Such a ray meets the light's object at distToLight and nowhere else, so a nearer hit is on another object and scene::hitLight's answer
 * is "blocked" whatever else the walk would find.  An update keeps the flags when it hands back every such light's object records
 * (and, if it carries matrices, the instance's two matrices) byte for byte and writes none of the light's vertices or triangles -- a
 * deformation tick of another mesh, other instances moving; 0 after any other update, until the next atn_upload_scene. */
uint32_t atn_planar_area_lights(atn_ctx* ctx);
uint32_t atn_tile_slots(atn_ctx* ctx);          /* identical on every rank: ceil(n_tiles / world) * 64 */
void* atn_stream(atn_ctx* ctx);                 /* hipStream_t all work is enqueued on */
int atn_synchronize(atn_ctx* ctx);

/* Scatter an all-gathered tile buffer (rank-major, world * atn_tile_slots float4, device memory)
 * into film_dev_out (float4[width*height], device memory; NULL = the context's own film). */
int atn_assemble_tiles(atn_ctx* ctx, const void* gathered_dev, int32_t world, void* film_dev_out);
/* Same, on a caller's HIP stream (hipStream_t; NULL = the context's): lets the exchange + assembly of frame f run
 * on a communication stream while the context's stream already renders frame f + 1. */
int atn_assemble_tiles_on(atn_ctx* ctx, const void* gathered_dev, int32_t world, void* film_dev_out, void* hip_stream);
int atn_download_film(atn_ctx* ctx, atn_vec4* out_host);
/* Checkpoint / resume of the progressive film (FilmProgressive's running mean + sample count in .w,
 * src/libaten/renderer/film.cpp:61-71): what atn_download_film returned is put back, and the next progressive
 * atn_render of that size continues from it exactly as if the earlier frames had run on this context. */
int atn_upload_film(atn_ctx* ctx, int32_t width, int32_t height, const atn_vec4* film_host);

/* Counters of the last atn_render with count_stats = 1:
 * {closest rays, shadow rays, shaded hits, closest node visits, closest triangle tests,
 *  shadow node visits, shadow triangle tests, 0}. */
int atn_get_stats(atn_ctx* ctx, uint64_t out[8]);
/* The per-pixel cost map of the last frame rendered with count_stats = 1: uint32 {BVH node visits, triangle tests}[h][w] of all
 * the pixel's walks (closest and shadow, every sample and bounce).  ≙ the heat map the reference builds from its per-path GPU
 * timer (PathTimeProfiler, src/libaten/renderer/pathtracing/path_time_profiler.h:15-60; ComputeTemperature maps it to colours) --
 * the deterministic quantity behind that time.  Pixels of other ranks' tiles are 0. */
int atn_download_path_cost(atn_ctx* ctx, uint32_t* out_host);

/* Kernel classes for atn_get_kernel_times. */
enum { ATN_K_GEN = 0, ATN_K_TRACE_CLOSEST = 1, ATN_K_SHADE = 2, ATN_K_TRACE_SHADOW = 3,
       ATN_K_ACCUM = 4, ATN_K_GATHER = 5,
       ATN_K_SVGF_PREPARE = 6, ATN_K_SVGF_TEMPORAL = 7, ATN_K_SVGF_VARIANCE = 8, ATN_K_SVGF_ATROUS = 9,
       ATN_K_TRACE_FUSED = 10,      /* shadow rays of bounce b + closest-hit rays of bounce b+1 in one launch */
       ATN_K_COUNT = 11,
       /* node-wide SVGF's two data movers (atn_mgpu_get_kernel_times only: atn_get_kernel_times keeps its ATN_K_COUNT entries) */
       ATN_K_SVGF_PACK = 11, ATN_K_SVGF_UNPACK = 12,
       ATN_K_MGPU_COUNT = 13 };
/* HIP-event time (ms) and launch count per kernel class, accumulated over every atn_render with
 * profile = 1 since the last atn_reset_kernel_times. */
int atn_get_kernel_times(atn_ctx* ctx, float ms[ATN_K_COUNT], uint32_t launches[ATN_K_COUNT]);
int atn_reset_kernel_times(atn_ctx* ctx);

/* Execution knob, no effect on results: the frame's paths are processed as up to `n` independent batches on
 * `n` HIP streams so that one batch's kernels fill the GPU during another's launch tails (default 3, automatically
 * fewer for small frames / shards; 1 = strictly one kernel at a time, which is what per-kernel timings of an
 * isolated kernel need). */
int atn_set_path_batches(atn_ctx* ctx, int32_t n);

/* Execution knob, no effect on results: how many consecutive atn_render frames may be in flight on the GPU at once
 * (1 .. 4, default 1).  With n > 1 the context keeps n banks of path state and streams and atn_render(f + 1) is enqueued
 * on another stream than frame f: the launch tails of one frame overlap the bulk of the next (what limits a small frame
 * -- one GPU's share of a sharded 1080p image -- is the ~0.13 ms tail of each of its depth + 1 trace launches, DESIGN.md
 * section 8).  Only the film orders the frames.  atn_stream / atn_tile_device then refer to the LAST rendered frame;
 * every other entry point first waits for all frames in flight. */
int atn_set_frames_in_flight(atn_ctx* ctx, int32_t n);
/* Diagnostics of the above: HIP streams share a few hardware queues and two streams on one queue run one after the other, so
 * atn_set_frames_in_flight MEASURES which of its bank streams run side by side and replaces the ones that do not (DESIGN.md
 * section 8).  *swaps = streams replaced so far; *concurrent: bit 0 = every pair of the current bank streams was measured
 * to overlap (re-measured by this call; 0 = fewer hardware queues than frames in flight), bit 1 = the side stream
 * (atn_side_stream), if it was handed out, overlaps with every bank stream.  Either may be NULL. */
int atn_bank_streams(atn_ctx* ctx, int32_t* swaps, int32_t* concurrent);
/* A stream for the CALLER's own work beside the frames in flight (a tile exchange, a display copy): created on first use and
 * chosen -- by the same measurement -- to run side by side with every bank stream when a hardware queue is left for it
 * (a stream the caller creates itself lands on SOME queue, possibly a bank's, and then waits behind that bank's kernels).
 * Owned by the context; NULL on failure.  Call after atn_set_frames_in_flight. */
void* atn_side_stream(atn_ctx* ctx);

/* Optional samplers, both off by default: they change the sample stream, i.e. they leave the parity path of
 * aten::PathTracing (every default-mode result still matches the CPU renderer).
 *   ibl_importance != 0: the IBL light is sampled from the luminance tables of the environment map --
 *       ImageBasedLight::preCompute (src/libaten/light/ibl.cpp:10-118) and the table sampler ImageBasedLight::sample
 *       (ibl.cpp:180-230) -- instead of light/ibl.h:98-100's cosine-hemisphere sampling; BSDF-sampled misses are weighted
 *       with the same density.
 *   tex_bilinear != 0: every texture lookup is aten::texture::AtWithBilinear (src/libaten/image/texture.cpp:77-125)
 *       instead of texture::at (the CUDA backend filters with tex2DLod, material/sample_texture.h:18-40). */
int atn_set_sampling_options(atn_ctx* ctx, int32_t ibl_importance, int32_t tex_bilinear);
/* Stage probe: n lookups of texture `texid` at uv_host[2n] -> out_host[4n], with the current texture mode. */
int atn_sample_texture(atn_ctx* ctx, int32_t texid, uint32_t n, const float* uv_host, float* out_host);

/* ---- one node, every GPU ------------------------------------------------------------------------
 * The reference renderer is single-device (idaten::Renderer, src/libidaten/kernel/renderer.h:17-179; its caller
 * src/device_renderer/main.cpp:133-149,196-204 makes one UpdateSceneData and one render(dst) per frame).  An
 * atn_mgpu keeps exactly that call shape and spreads the frame over the node: one context + one host worker thread
 * per shard, the scene replicated, the screen cut into 8x8-pixel tiles (tile t -> shard t % N, seeds and pixel indices
 * global, so the image does not depend on N), and per frame ONE exchange: every shard pushes its tile buffer to
 * shard 0's device with a peer copy over xGMI and shard 0 scatters them into the full frame.  The film of frame f is
 * assembled while frame f + 1 renders (two gather buffers, events both ways).
 *
 * devices: HIP ordinals of the shards, n_devices entries; NULL = ordinals 0 .. n_devices-1, and NULL with
 * n_devices <= 0 = every visible device.  An ordinal may repeat (shards sharing a GPU): with that the whole N > 1 path
 * runs on a one-GPU machine.  All calls return 0 or a negative atn_status; none throws. */
typedef struct atn_mgpu atn_mgpu;
int atn_mgpu_create(atn_mgpu** out, const int32_t* devices, int32_t n_devices);
void atn_mgpu_destroy(atn_mgpu* mg);
const char* atn_mgpu_last_error(atn_mgpu* mg);
int32_t atn_mgpu_shard_count(atn_mgpu* mg);
int32_t atn_mgpu_shard_device(atn_mgpu* mg, int32_t shard);
/* ≙ UpdateSceneData / updateBVH / updateCamera / initSampler on every shard (uploads run in parallel). */
int atn_mgpu_upload_scene(atn_mgpu* mg, const atn_scene_desc* scene);
int atn_mgpu_update_tlas(atn_mgpu* mg, const atn_object_param* objects, uint32_t n_objects,
                         const atn_mat4* matrices, uint32_t n_matrices,
                         const atn_bvh_node* top_nodes, uint32_t n_top_nodes);
/* atn_tlas_rebuild on every shard */
int atn_mgpu_tlas_rebuild(atn_mgpu* mg, const atn_object_param* objects, uint32_t n_objects,
                          const atn_mat4* matrices, uint32_t n_matrices, uint32_t flags);
int atn_mgpu_update_geometry(atn_mgpu* mg, const atn_vec4* vtx_pos, const atn_vec4* vtx_nml, uint32_t n_vertices, uint32_t vtx_offset,
                             const atn_triangle_param* triangles, uint32_t n_triangles, uint32_t tri_offset);
int atn_mgpu_lbvh_rebuild_list(atn_mgpu* mg, uint32_t list_index, uint32_t tri_offset, uint32_t n_triangles,
                               const float bbox_min[3], const float bbox_max[3]);
/* the scene edits (atn_update_materials and its kin, above) on every shard */
int atn_mgpu_update_materials(atn_mgpu* mg, const atn_material_param* materials, uint32_t n, uint32_t first);
int atn_mgpu_update_lights(atn_mgpu* mg, const atn_light_param* lights, uint32_t n, uint32_t first, int32_t npr_target);
int atn_mgpu_update_texture(atn_mgpu* mg, int32_t texid, const atn_texture_desc* tex);
int atn_mgpu_update_rendering_config(atn_mgpu* mg, const atn_scene_rendering_config* config);
int atn_mgpu_update_camera(atn_mgpu* mg, const atn_camera_param* camera);
int atn_mgpu_init_sampler(atn_mgpu* mg, int32_t width, int32_t height, int32_t seed);
int atn_mgpu_set_random(atn_mgpu* mg, const uint32_t* seeds, uint32_t n);
/* ≙ idaten::PathTracing::render for the whole node.  out_host NULL: returns when the frame is enqueued; the
 * assembled film (float4[w*h], row 0 = bottom) is atn_mgpu_film_device on shard 0's device, complete after
 * atn_mgpu_synchronize.  out_host != NULL: returns with the frame in host memory. */
int atn_mgpu_render(atn_mgpu* mg, const atn_destination* dst, atn_vec4* out_host);
int atn_mgpu_reset(atn_mgpu* mg);
int atn_mgpu_synchronize(atn_mgpu* mg);
void* atn_mgpu_film_device(atn_mgpu* mg);
int atn_mgpu_download_film(atn_mgpu* mg, atn_vec4* out_host);
/* atn_set_frames_in_flight on every shard. */
int atn_mgpu_set_frames_in_flight(atn_mgpu* mg, int32_t n);
/* atn_set_regeneration on every shard; atn_render_burst on every shard followed by ONE exchange of the tiles (a progressive film is
 * looked at after the burst: its tiles travel once per burst, not once per frame). */
int atn_mgpu_set_regeneration(atn_mgpu* mg, int32_t mode);
/* atn_set_sphere_intersection on every shard (read by the next atn_mgpu_upload_scene / atn_mgpu_update_tlas) */
int atn_mgpu_set_sphere_intersection(atn_mgpu* mg, int32_t mode);
int atn_mgpu_render_burst(atn_mgpu* mg, const atn_destination* dst, int32_t n_frames, atn_vec4* out_host);
/* Node-wide SVGF (docs/MGPU_SVGF.md): atn_svgf_render (below) with the path pass -- most of the frame -- spread over the shards.  Every
 * shard runs the path pass on its tiles; shards 1 .. N-1 pack their pixels of the four planes the path pass hands to the filters
 * (contributions, normal+depth, albedo+id, primary hit positions: 64 B per pixel) and push them to shard 0's device in one peer copy
 * each; shard 0 scatters them into its own planes and runs the filter passes there.  The result -- out_host, stages_host, every
 * plane of atn_mgpu_svgf_download -- is byte-equal to atn_svgf_render on one unsharded context given the same calls in the same
 * order, whatever N is.  compute_motion 0 (the plane of atn_mgpu_svgf_set_motion_depth) and != 0 (computed from the primary hits),
 * destination.sample >= 1, and frame == 0 taking the first-frame path, as atn_svgf_render; compute_motion = 2 is
 * ATN_ERR_UNSUPPORTED (the geometry history has no node-wide form yet).  Regeneration does not apply.  Returns once everything is
 * enqueued unless a host pointer is given; ordered by events only, so with atn_mgpu_set_frames_in_flight > 1 frame f + 1's path
 * pass and exchange overlap frame f's filters.  On a failure atn_mgpu_last_error names the shard; the shards may then disagree about
 * the frame they are at, so the caller must atn_mgpu_svgf_reset before the next atn_mgpu_svgf_render.  May be mixed with
 * atn_mgpu_render / atn_mgpu_render_burst on one atn_mgpu as atn_svgf_render with atn_render on one context.  The display tail
 * (atn_taa_resolve) has no node-wide form. */
int atn_mgpu_svgf_render(atn_mgpu* mg, const atn_destination* dst, int32_t compute_motion, atn_vec4* out_host, atn_vec4* stages_host);
/* atn_svgf_set_motion_depth / _set_atrous_iterations / _set_dilate_temporal_weight on shard 0 (the filters run there); atn_svgf_reset
 * on every shard; atn_svgf_download and atn_svgf_output_device of shard 0's planes (`which` as atn_svgf_download). */
int atn_mgpu_svgf_set_motion_depth(atn_mgpu* mg, const atn_vec4* motion_depth, uint32_t n);
int atn_mgpu_svgf_reset(atn_mgpu* mg);
int atn_mgpu_svgf_set_atrous_iterations(atn_mgpu* mg, int32_t n);
int atn_mgpu_svgf_set_dilate_temporal_weight(atn_mgpu* mg, int32_t on);
int atn_mgpu_svgf_download(atn_mgpu* mg, int32_t which, atn_vec4* out_host);
void* atn_mgpu_svgf_output_device(atn_mgpu* mg);
/* atn_get_kernel_times / atn_reset_kernel_times of one shard / of every shard, with the two classes of the exchange: ATN_K_SVGF_PACK
 * on shards 1 .. N-1, ATN_K_SVGF_UNPACK on shard 0 (frames rendered with destination.profile = 1).  Waits for the frames in flight. */
int atn_mgpu_get_kernel_times(atn_mgpu* mg, int32_t shard, float ms[ATN_K_MGPU_COUNT], uint32_t launches[ATN_K_MGPU_COUNT]);
int atn_mgpu_reset_kernel_times(atn_mgpu* mg);

/* ---- SVGF (next tier, BASELINE config 5) -------------------------------------------------------
 * ≙ aten::SVGFRenderer (src/libaten/renderer/svgf/svgf.{h,cpp}): the path pass with AOV outputs
 * (SVGFRenderer::Shade / ShadeMiss with AOV spans) followed by the svgf_impl.h passes as HIP kernels --
 * PrepareForDenoise, TemporalReprojection + AccumulateMoments (frame > 0), EstimateVariance,
 * atrous_iter_cnt x (3x3 Gauss of the variance + ExecAtrousWaveletFilter + PostProcessForAtrousFilter),
 * CopyFromTeporaryColorBufferToAov -- with the AOV / moment buffers of two frames resident in HBM.
 * `dst->frame == 0` takes the first-frame path (svgf.cpp:519-525,543-551).  One context renders the whole frame (a context with
 * a screen shard is refused: the filters' footprints cross tiles); the node-wide form is atn_mgpu_svgf_render, above.
 *
 * out_host (may be NULL): what dst.buffer holds when OnRender returns (the last a-trous iteration's
 * albedo-multiplied colour), vec4[w*h], row 0 = bottom.  stages_host (may be NULL): 3 x vec4[w*h], the
 * values OnRender puts after the path pass, the temporal pass and the variance pass.
 * compute_motion != 0: the motion/depth buffer is computed from the primary hits and the current/previous
 * camera matrices (MatricesForRendering, pt_params.h:150-185) -- the compute pass that stands in for the
 * reference's GL raster pass (src/shader/ssrt_fs.glsl:31-47); 0: use atn_svgf_set_motion_depth's buffer;
 * 2: the same pass with the geometry's own motion (atn_set_geometry_motion, below). */
int atn_svgf_render(atn_ctx* ctx, const atn_destination* dst, int32_t compute_motion,
                    atn_vec4* out_host, atn_vec4* stages_host);
/* ≙ SVGFRenderer::SetMotionDepthBuffer (svgf.cpp:441-450): {motion.xy in screen fractions, depth, 1}. */
int atn_svgf_set_motion_depth(atn_ctx* ctx, const atn_vec4* motion_depth, uint32_t n);
/* Forget the frame history (AOV sets, moments, previous camera matrices). */
int atn_svgf_reset(atn_ctx* ctx);
/* SVGFParams::atrous_iter_cnt (svgf_types.h:72), default 5. */
int atn_svgf_set_atrous_iterations(atn_ctx* ctx, int32_t n);
/* Optional pass, off by default (the CPU SVGFRenderer, the parity target, never runs it; the CUDA twin does, right after
 * temporal reprojection: src/libidaten/svgf/svgf_tp.cu:150-216): RecomputeTemporalWeightFromSurroundingPixels
 * (src/libaten/renderer/svgf/svgf_impl.h:386-423) -- a non-background pixel's temporal weight becomes the minimum over
 * its 3x3 neighbourhood, every tap reading the weights the pass started with. */
int atn_svgf_set_dilate_temporal_weight(atn_ctx* ctx, int32_t on);
/* Parity probe.  which: 0-3 SVGFParams::GetCurrAovBuffer() as the state stands (OnRender toggles at its end, so
 * this is the set the NEXT frame writes: normal+depth, albedo+meshid, colour+variance, moments+temporal weight),
 * 4-7 GetPrevAovBuffer() (the set the last frame wrote), 8 temporary colour, 9 motion/depth, 10 primary hit
 * position, 11/12 a-trous ping-pong buffers, 13 output, 14 contributions. */
int atn_svgf_download(atn_ctx* ctx, int32_t which, atn_vec4* out_host);

/* ---- Geometry motion vectors (docs/MOTION.md) ------------------------------------------------------------------------------
 * ≙ the G-buffer pass of drawSceneForGBuffer for moving geometry (src/shader/ssrt_deformable_vs.glsl, ssrt_vs.glsl: a previous
 * position per vertex, a previous local-to-world matrix per object).  The context keeps a GEOMETRY HISTORY: the scene's vertex
 * positions and matrices as the last frame rendered with compute_motion = 2 saw them (equal to the scene after atn_upload_scene and
 * when tracking is switched on).  Such a frame projects every primary hit through the current camera from where it is and through
 * the previous camera from where the history has it; then the history takes over the ranges the updates since wrote.
 *   atn_set_geometry_motion: on != 0 allocates the history and starts tracking (default off; waits for the frames in flight);
 *                            0 frees it.  ATN_ERR_UNSUPPORTED after atn_scene_device_arrays (which also switches tracking off).
 *   compute_motion = 2 (atn_svgf_render, atn_restir_render): ATN_ERR_INVALID_ARG while tracking is off; ATN_ERR_UNSUPPORTED for
 *                            atn_svgf_denoise (no path pass: no ids) and for atn_svgf_render with destination.sample != 1.
 *   ids plane: atn_svgf_download which = 15, atn_restir_download which = 8, of the last frame if it was rendered with
 *                            compute_motion = 2: atn_vec4[w*h] {object id (int bits; -1 = miss), triangle id (int bits), a, b}.
 * For tests (like atn_skin_download: not part of what an application needs):
 *   atn_geometry_motion_stats: {motion passes, range copies into the history, float4s copied} since the context was created.
 *   atn_geometry_motion_matrices: the world-to-clip matrices (row-major) of this frame's and the previous frame's camera that the
 *                            last motion pass used.
 * SVGF and ReSTIR frames of a context share the one history.  Additive entry points: atn_abi_version stays 3. */
int atn_set_geometry_motion(atn_ctx* ctx, int32_t on);
int atn_geometry_motion_stats(atn_ctx* ctx, uint64_t* out3);
int atn_geometry_motion_matrices(atn_ctx* ctx, float* w2c16, float* prev_w2c16);

/* ---- ReSTIR (idaten::ReSTIRPathTracing; docs/RESTIR.md) ------------------------------------------------------------------
 * Many-light direct lighting at the primary hit with reservoir resampling (initial candidates, temporal and spatial reuse); the
 * bounces behind it are the path tracer's.  Frame-persistent state lives in the context (atn_restir_reset forgets it).
 *   atn_restir_set_options: mode 0 = initial candidates only, 1 = temporal + spatial (default), 2 = spatial, 3 = temporal;
 *                           n_candidates in [1, 32] (default 32)
 *   atn_restir_render: one frame (destination.sample must be 1); the film follows atn_render's progressive / overwrite rules.
 *                      compute_motion != 0: motion/depth from the primary hits (as atn_svgf_render), else the buffer of
 *                      atn_restir_set_motion_depth.  ATN_ERR_UNSUPPORTED for sample != 1, a screen shard with world > 1, path
 *                      regeneration, relaxed shade math, count_stats and toon materials.
 *   atn_restir_capture: keep the stage buffers of the next frames (tests)
 *   atn_restir_download: which = 0 / 1 / 2 reservoirs after the shade / temporal (visibility) / spatial pass, float[w*h][5]
 *                        {y, M, W, w_sum, target_pdf} (capture on); 3 the infos, atn_vec4[4][w*h] {nml, mtrl id bits} {wi, u}
 *                        {p, v} {pre_sampled_r, mesh id bits, hit, 0}; 4 AOV normal+depth; 5 AOV albedo+mesh id; 6 the
 *                        motion-depth the last frame used (atn_vec4[w*h]: the caller's, or the one compute_motion computed -- it
 *                        never overwrites the caller's); 7 the CMJ dimension of every pixel after bounce 0's passes, uint32[w*h].
 *                        0-2 and 7 only for a frame rendered with capture on. */
int atn_restir_set_options(atn_ctx* ctx, int32_t mode, int32_t n_candidates);
int atn_restir_render(atn_ctx* ctx, const atn_destination* dst, int32_t compute_motion, atn_vec4* out_host);
int atn_restir_set_motion_depth(atn_ctx* ctx, const atn_vec4* motion_depth, uint32_t n);
int atn_restir_reset(atn_ctx* ctx);
int atn_restir_capture(atn_ctx* ctx, int32_t on);
int atn_restir_download(atn_ctx* ctx, int32_t which, void* out_host);

/* ---- NPR feature lines (aten::NprPathTracer / idaten::NPRPathTracing; docs/NPR.md) ------------------------------------------
 * The path tracer's sample loop with 8 sample rays per path that find feature lines (mesh, albedo, normal and depth edges) around
 * the path's query ray; a found line sets the path's contribution to the MIS-weighted line colour and ends the path.  Settings:
 * atn_scene_rendering_config.feature_line (atn_feature_line_config) and atn_material_param.feature_line (atn_feature_line_mtrl).
 *   atn_npr_render: one frame; the film follows atn_render's progressive / overwrite rules.  ATN_ERR_UNSUPPORTED for a config
 *                   with feature lines off, StencilType::STENCIL materials and alpha blending with a material whose alpha may be
 *                   < 1 (both unless atn_npr_set_skip_through(1)), CarPaint materials, a screen shard with world > 1, path regeneration, relaxed shade math and count_stats.
 *   atn_npr_reset: the film and the sample-ray state start over (a fresh context's)
 *   atn_npr_capture: keep the stage buffers of the next frames (tests)
 *   atn_npr_download: which = 0 the line decision per pixel, atn_vec4[w*h] {found, bounce, closest distance, 0} of the frame's
 *                     last sample that found one; 1 the sample-ray descriptors after bounce 0, atn_vec4[w*h][8] {u, v, live, 0};
 *                     2 the disc after bounce 0, atn_vec4[w*h][2] {center, radius} {normal, accumulated distance}; 3 the CMJ
 *                     dimension after bounce 0, uint32[w*h].  All for a frame rendered with capture on.
 *   atn_npr_set_skip_through: AdvanceNPRPath's look-through (docs/NPR_ADVANCE.md).  mode 0 (default): atn_npr_render refuses STENCIL
 *                     materials and alpha blending with an alpha that may be < 1, as above.  mode 1: it renders them -- behind a
 *                     STENCIL surface the path looks for a front-facing ALWAYS surface (CheckStencil), behind a surface with
 *                     alpha < 1 it goes on with the surface's colour blended in (CheckMaterialTranslucentByAlpha); a scene that
 *                     needs neither renders with the kernels of mode 0, byte for byte.  Mode 1 on a scene that needs the look-through
 *                     refuses atn_npr_shadow_set_mode(1), hatching included (ATN_ERR_UNSUPPORTED).  Other values: ATN_ERR_INVALID_ARG.
 *   atn_npr_advance_download: the look-through's stage buffer of the last frame (capture on, mode 1, a scene that needs it), after
 *                     bounce 0: atn_vec4[w*h][2] {the check that said true: 0 none, 1 stencil, 2 alpha; walks done; the answer: the
 *                     triangle id, or -1 for a miss; is_singular} {alpha_blend.throughput.rgb, alpha_blend.transmission}
 * Additive entry points: atn_abi_version stays 3. */
int atn_npr_render(atn_ctx* ctx, const atn_destination* dst, atn_vec4* out_host);
int atn_npr_reset(atn_ctx* ctx);
int atn_npr_capture(atn_ctx* ctx, int32_t on);
int atn_npr_download(atn_ctx* ctx, int32_t which, void* out_host);
int atn_npr_set_skip_through(atn_ctx* ctx, int32_t mode);
int atn_npr_advance_download(atn_ctx* ctx, void* out_host);

/* ---- Volume rendering: path tracing through homogeneous and grid media (aten::VolumePathTracing / idaten::VolumeRendering; docs/VOLUME.md)
 * Materials with is_medium set carry a medium (atn_medium_param): type ATN_MTRL_VOLUME is a pure boundary the ray passes through,
 * any other type a surface with a scattering interior.  A path runs at most 8 iterations (the reference's cap); light connections
 * walk through medium boundaries and collect transmittance.
 *   atn_volume_set_grids: n dense float grids (host arrays, copied) that a medium names by atn_medium_param.grid_idx; n = 0 drops them.
 *                      A medium with 0 <= grid_idx < n is heterogeneous: delta tracking against atn_medium_param.majorant samples its
 *                      free flight, ratio tracking its connections (HeterogeneousMedium, volume/medium.cpp:58-202).  The world box is
 *                      origin .. origin + dim * voxel_size; a point maps to the voxel floor((p - origin) * (1 / voxel_size)); outside
 *                      the box the density is 0.  Waits for frames in flight; the grids outlive atn_update_*, atn_upload_scene drops
 *                      them.  A grid or medium that cannot be traced is refused by atn_volume_render, not here.
 *   atn_volume_render: one frame; the film follows atn_render's progressive / overwrite rules.  ATN_ERR_UNSUPPORTED for a medium
 *                      with grid_idx >= the number of grids set; a grid medium with sigma_a != 0, with a majorant that is not finite,
 *                      <= 0, below sigma_s * max density, or above 1024 / box diagonal; a grid with a dim <= 0, a voxel_size that is
 *                      not finite or <= 0, or a density that is not finite or < 0; sigma_a + sigma_s <= 0, a screen shard with world > 1, path
 *                      regeneration, relaxed shade math, count_stats, alpha blending with a material whose alpha may be < 1,
 *                      StencilType::STENCIL materials, CarPaint and Toon / Stylized materials.  A scene without media renders.
 *   atn_volume_reset: the film starts over (a fresh context's)
 *   atn_volume_capture: keep the per-pixel state after iteration `iteration` (0..7) of sample 0 of the next frames; < 0: off
 *   atn_volume_download: which = 0 uint32[w*h][4] {flags, depth_count, stack size, CMJ dimension}; flags: 1 processed, 2 hit,
 *                        4 free flight sampled, 8 absorbed, 16 scattered, 32 passed through a boundary, 64 connection made,
 *                        256 terminated;  1 uint32[w*h][4] the medium stack, eight 16-bit ids, the newest in the low half of word 0;
 *                        2 atn_vec4[w*h][2] {next ray org, sampled distance s} {next ray dir, hit distance};
 *                        3 atn_vec4[w*h][3] the connection {org, t_max} {dir, transmittance} {segments, visible, 0, 0};
 *                        4 uint32[4] the last frame's counters {pushes dropped on a full stack, connections that crossed 64
 *                        boundaries, connections, segments} (needs no capture);
 *                        5 uint32[2] {grid flights, grid connections stopped after 16384 tracking steps} (needs no capture).
 *                        With grid media, the flight's step count is in bits 16-30 of the flags, and the connection's third vector
 *                        is {segments, visible, ratio-tracking steps, final dimension of the connection's sample stream}.
 *   atn_volume_phase_table: HenyeyGreensteinPhaseFunction::SampleDirection(r1, r2, g, w) -> out_dir[3 n] and Evaluate(g, w, wo) ->
 *                        out_eval[n] for n cases (host arrays; w, wo: float[3 n])
 * Additive entry points: atn_abi_version stays 3. */
typedef struct atn_volume_grid {
    int32_t dim[3];             /* voxels along x, y, z */
    float origin[3];            /* the world position of voxel (0, 0, 0)'s low corner */
    float voxel_size;
    const float* density;       /* host floats, x fastest: dim[0] * dim[1] * dim[2] values */
} atn_volume_grid;
int atn_volume_set_grids(atn_ctx* ctx, const atn_volume_grid* grids, uint32_t n);
int atn_volume_render(atn_ctx* ctx, const atn_destination* dst, atn_vec4* out_host);
int atn_volume_reset(atn_ctx* ctx);
int atn_volume_capture(atn_ctx* ctx, int32_t iteration);
int atn_volume_download(atn_ctx* ctx, int32_t which, void* out_host);
int atn_volume_phase_table(atn_ctx* ctx, float g, uint32_t n, const float* w, const float* r1, const float* r2, const float* wo,
                           float* out_dir, float* out_eval);

/* ---- Ambient occlusion (aten::AORenderer / idaten::AORenderer; docs/AO.md) ----------------------------------------------------
 * Per pixel: the primary hit, num_rays cosine-weighted AO rays of length `radius` from it, ao = sum of t / radius * c / pdf over the
 * rays that hit (a ray that misses SETS the value to 1), / num_rays; hits on translucent-by-alpha materials are skipped through, up to
 * 10 walks per ray.  One sample per pixel.
 *   atn_ao_set_params: num_rays 1..64 (default 1), radius > 0 and finite (default 1.0), filter 0 / 1 (default 0: RenderAO; 1:
 *                      RenderAOWithBilateralFilter's two 7-tap depth-aware passes and its halving).  ATN_ERR_INVALID_ARG otherwise.
 *   atn_ao_render: one frame; reads dst->frame, width, height, progressive (atn_render's film rules) and break_on_terminate; sample
 *                  and maxDepth are ignored.  break_on_terminate = 1 is the CPU renderer as written: in every row the pixels from the
 *                  first primary miss on are NOT written and keep what the film held (zero in a fresh context and after
 *                  atn_ao_reset) -- the Cornell box at 4:3 has a miss at x = 0 of every row, so nothing is written there.
 *                  break_on_terminate = 0 is idaten's rule: a primary miss is 1.0 and every pixel is written.  ATN_ERR_UNSUPPORTED
 *                  for a screen shard with world > 1, path regeneration, relaxed shade math, count_stats, CarPaint materials, and
 *                  filter = 1 together with break_on_terminate = 1.
 *   atn_ao_reset: the film and the AO planes start over (a fresh context's)
 *   atn_ao_capture: keep the first AO ray and its answer of the next frames (tests)
 *   atn_ao_download: which = 0 uint32[w*h] the state word, 0 not rendered / 1 hit / 2 miss; 1 float[w*h] the AO value handed to the
 *                    film (before the filter); 2 float[w*h] the primary hit's t (inf: a miss); 3 uint32[h] the row's first primary
 *                    miss x (0xffffffff: none) -- all of the last frame, pixels not rendered keeping earlier content;  with capture
 *                    on: 4 atn_vec4[w*h][2] the first AO ray {org, 0} {dir, 0}; 5 atn_vec4[w*h] its answer {0 miss | 1 hit | 2 ten
 *                    skip-throughs, t, c, skip-throughs}, of pixels in state 1.
 * Additive entry points: atn_abi_version stays 3. */
int atn_ao_set_params(atn_ctx* ctx, int32_t num_rays, float radius, int32_t filter);
int atn_ao_render(atn_ctx* ctx, const atn_destination* dst, atn_vec4* out_host);
int atn_ao_reset(atn_ctx* ctx);
int atn_ao_capture(atn_ctx* ctx, int32_t on);
int atn_ao_download(atn_ctx* ctx, int32_t which, void* out_host);
/* ---- The NPR shadow pre-pass (aten::NprPathTracer::OnRender's first pass, src/libaten/renderer/npr/npr.cpp:284-349,399-447;
 * idaten::NPRPathTracing::onShadeByShadowRay, src/libidaten/npr/npr_pathtracing.cu:211-281,446-476,521-605; docs/NPR_SHADOW.md) ----
 * The screen-space shadow texture Toon / StylizedBrdf materials multiply their band with (ToonParameter::stylized_shadow,
 * material/toon.cpp:148-160), made per frame from the frame's own rays: per pixel the bounce-0 NEE shadow ray of sample 0 (the ray
 * PathTracing::shade casts, pathtracing.cpp:91-236, with the path's termination flag forced off, npr.cpp:305-307), whether it reached
 * its light (HitTestToTargetLight, pathtracing_impl.h:266-393), and that bit filtered along the row by
 * ApplyBilateralFilter<ShadowRay, float, true, 5> with coefficients (2, 2) (aorenderer_impl.h:138-191; 11 taps, the depth the
 * primary hit's t).
 *   atn_npr_shadow_set_mode: 0 (default) Toon shading reads the texture uploaded with the scene (atn_scene_desc::screen_space_texture);
 *                    1 atn_render and atn_npr_render first run the pre-pass for the frame's camera and the frame's Toon shading reads
 *                    its plane.  A scene without a material that enables the term skips the pre-pass.  Other values:
 *                    ATN_ERR_INVALID_ARG.  While the mode is 1: ATN_ERR_UNSUPPORTED for a screen shard with world > 1, path
 *                    regeneration, atn_render_burst, relaxed shade math, count_stats and CarPaint materials.  The SVGF, ReSTIR, volume
 *                    and AO frames ignore the mode.
 *   atn_npr_shadow_download: the planes of the last frame that ran the pre-pass, n = width * height floats, row-major: which = 0 the
 *                    filtered plane; 1 the bit as 0.0 / 1.0; 2 the primary hit's t (inf: a miss).  Waits for that frame.
 *                    ATN_ERR_INVALID_ARG before such a frame and for another n.
 *   atn_npr_shadow_filter: the row filter alone over host planes lit / depth [h][w] -> out_host [h][w]; w, h 1..16384.
 * Additive entry points: atn_abi_version stays 3. */
int atn_npr_shadow_set_mode(atn_ctx* ctx, int32_t mode);
int atn_npr_shadow_download(atn_ctx* ctx, int32_t which, float* out_host, uint32_t n);
int atn_npr_shadow_filter(atn_ctx* ctx, const float* lit, const float* depth, int32_t w, int32_t h, float* out_host);
/* ---- NPR hatching shadows (idaten::NPRPathTracing's HatchingShadowBase x HatchingShadowDirection, src/libidaten/npr/
 * npr_pathtracing.h:14-26, npr_pathtracing.cu:283-347,351-386,519-605; docs/NPR_HATCHING.md) ----
 * What the pre-pass of atn_npr_shadow_set_mode(1) filters, and how.
 *   atn_npr_hatching_set: base 0 = AO (ShandeByAO at the primary hit, ao_num_rays rays of ao_radius, drawn from the AO renderer's own
 *                    sampler), 1 = ShadowRay (default: the bounce-0 lit bit).  direction 0 None, 1 Horizontal (default), 2 Vertical,
 *                    3 Orthogonal, 4 Cross (Horizontal x Vertical), 5 OrthogonalCross (diagonal x anti-diagonal); the two-step
 *                    products are darkened by `v < 1 ? v * 0.5 : v`.  ao_num_rays 1..64, ao_radius > 0 and finite (read with base 0
 *                    only).  Anything else: ATN_ERR_INVALID_ARG, nothing changes.  Waits for the frames in flight; takes effect for
 *                    the mode-1 frames of atn_render and atn_npr_render; context state, kept across atn_upload_scene.  The scene's
 *                    enable_shadowray_base_stylized_shadow is not overridden in either base.  With base 0 a frame that would list more
 *                    than 2^28 AO rays is ATN_ERR_UNSUPPORTED.
 *   atn_npr_hatching_get: the four settings (null pointers are skipped).
 *   atn_npr_hatching_filter: the filter of `direction` alone over host planes src / depth [h][w] -> out_host [h][w]; w, h 1..16384.
 *   atn_npr_hatching_download: planes of the last frame that ran the pre-pass, n = width * height floats: which = 0 the unfiltered
 *                    source plane (AO values with base 0, the bit as 0.0 / 1.0 with base 1), 1 the first step's plane (the final plane
 *                    of a one-step direction).  ATN_ERR_INVALID_ARG before such a frame and for another n.
 * atn_npr_shadow_download(0) is the final plane whatever the settings and (2) the depth; (1) is ATN_ERR_INVALID_ARG after a base-0
 * frame (there is no bit).  Additive entry points: atn_abi_version stays 3. */
int atn_npr_hatching_set(atn_ctx* ctx, int32_t base, int32_t direction, int32_t ao_num_rays, float ao_radius);
int atn_npr_hatching_get(atn_ctx* ctx, int32_t* base, int32_t* direction, int32_t* ao_num_rays, float* ao_radius);
int atn_npr_hatching_filter(atn_ctx* ctx, const float* src, const float* depth, int32_t w, int32_t h, int32_t direction, float* out_host);
int atn_npr_hatching_download(atn_ctx* ctx, int32_t which, float* out_host, uint32_t n);
/* The filter passes alone (everything of OnRender after the sample loop, svgf.cpp:515-637) on whatever the
 * path pass -- or atn_svgf_upload -- left in the buffers: contributions (which = 14: contrib.xyz, sample count),
 * the current AOVs (0, 1), primary hit positions (10), motion/depth (9).  This is how a caller that already has a
 * noisy frame and a G-buffer uses the denoiser, and how the parity tests feed both sides identical inputs. */
int atn_svgf_denoise(atn_ctx* ctx, const atn_destination* dst, int32_t compute_motion,
                     atn_vec4* out_host, atn_vec4* stages_host);
int atn_svgf_upload(atn_ctx* ctx, int32_t which, int32_t width, int32_t height, const atn_vec4* host);
void* atn_svgf_output_device(atn_ctx* ctx);

/* ---- The display tail: temporal anti-aliasing and gamma (aten::TAA + aten::GammaCorrection; docs/TAA.md) ---------------------------
 * ≙ the two post-processes svgf_renderer and deformation_renderer put behind the renderer (src/libaten/filter/taa.{h,cpp},
 * src/shader/taa_fs.glsl, src/shader/gamma_fs.glsl), as ONE kernel launch per frame: TAA from the frame's colour, the history and the
 * motion/depth plane; the history write (the TAA output IS the next frame's history); pow(rgb, 1 / gamma) clamped to [0, 1] as RGBA8
 * (R in the low byte, round to nearest) and, when asked for, as float4.  The gamma planes are never fed back.
 *   atn_taa_resolve: source 0 = the output and motion/depth plane of the last atn_svgf_render / atn_svgf_denoise frame, 1 = the film
 *                    and motion/depth plane of the last atn_restir_render frame, 2 = the planes of atn_taa_upload.  Enqueued behind
 *                    the frame that produced the source and ordered against the next frame on the device; the host waits only when
 *                    an output pointer is given (out_rgba32f: atn_vec4[w*h], out_rgba8: uint32[w*h]; either may be NULL; the float
 *                    gamma plane is written only when out_rgba32f is given).  enable = 0: every pixel passes through (the current
 *                    texel, alpha 1) and the history still advances.  The first frame after atn_taa_reset, a size change or context
 *                    creation has no history and passes through as well.  ATN_ERR_INVALID_ARG for gamma <= 0 or not finite, a size
 *                    outside 1 .. 16384 per side, source 0 / 1 without a frame of that renderer or with another size, source 2 without
 *                    both planes uploaded at that size.  (A frame without a motion/depth plane cannot exist: atn_svgf_render and
 *                    atn_restir_render refuse compute_motion = 0 without a caller's plane themselves.)
 *   atn_taa_upload:  which = 0 the colour, 1 the motion/depth plane {prev - cur in screen fractions, depth (< 0: a miss), 1}, 2 the
 *                    history (at a new size it starts a new history).  For tests and callers with a renderer of their own.
 *   atn_taa_download: which = 0 the TAA output (= the new history), 1 the history the last frame read (meaningful when it had one),
 *                    2 the gamma plane as atn_vec4[w*h] (if the last resolve asked for it), 3 as RGBA8 uint32[w*h].
 *   atn_taa_reset:   forget the history.  atn_svgf_reset, atn_restir_reset and atn_upload_scene do NOT; a size change does.
 *   atn_taa_output_device / atn_taa_rgba8_device: the last frame's TAA output (float4[w*h]) / RGBA8 plane in device memory (NULL
 *                    before the first atn_taa_resolve); the output pointer changes every frame (ping-pong).
 * One GPU only: atn_mgpu_* has no form of it.  Additive entry points: atn_abi_version stays 3. */
int atn_taa_resolve(atn_ctx* ctx, int32_t source, int32_t width, int32_t height, int32_t enable, float gamma,
                    atn_vec4* out_rgba32f, uint32_t* out_rgba8);
int atn_taa_upload(atn_ctx* ctx, int32_t which, int32_t width, int32_t height, const atn_vec4* host);
int atn_taa_download(atn_ctx* ctx, int32_t which, void* out_host);
int atn_taa_reset(atn_ctx* ctx);
void* atn_taa_output_device(atn_ctx* ctx);
void* atn_taa_rgba8_device(atn_ctx* ctx);

/* ---- stage entry points (parity tests; each mirrors one reference function) ---------------- */
/* GeneratePath for every pixel (src/libaten/renderer/pathtracing/pathtracing_impl.h:65-110). */
int atn_generate_paths(atn_ctx* ctx, int32_t width, int32_t height, int32_t sample, uint32_t frame, atn_ray* out_host);
/* ThreadedBvhTraverser::Traverse<Closest> (src/libaten/accelerator/threaded_bvh_traverser.h:98-304).
 * stats_out (optional): {node visits, triangle tests}. */
int atn_trace_closest(atn_ctx* ctx, const atn_ray* rays_host, uint32_t n, float t_min, float t_max,
                      atn_intersection* out_host, uint64_t* stats_out);
/* HitShadowRay -> HitTestToTargetLight -> scene::hitLight (pathtracing_impl.h:266-393, scene/scene.h:64-134) for n caller-given shadow
 * rays, through the PRODUCTION shadow kernels: the probe fills path buffers of its own as the shade stage leaves them (sh_o, sh_d, sh_c
 * with a known contribution, the shadow queue and its count), launches through the launchers the renderers use, on the walk the uploaded
 * scene calls for (ATEN_AMD_TRACE forces one), and reads each verdict back from the plane the flavour adds to.  Query i lives in slot
 * 2 i + 1 and the queue is shuffled; the slots in between must come back untouched (checked on the device: ATN_ERR_HIP otherwise).
 *   flavour 0 "fused":    the shadow half of the fused trace launch (no closest-hit rays beside it)
 *           1 "counted":  the unfused shadow kernel of counted frames
 *           2 "deferred": as 0 in a deferred-NEE frame: the verdict is the slot's flag word, `contrib` stays zero
 *           3 "regen":    the regenerated pool's launch; a query with flags bit 1 adds to `pend`, every other to `contrib`
 * out_visible[i] = 1 when query i's contribution was added.  ATN_ERR_NO_SCENE without a scene, ATN_ERR_INVALID_ARG for null pointers,
 * an unknown flavour or a light index outside the scene's lights, ATN_ERR_UNSUPPORTED for a scene without lights; n == 0 is a no-op. */
int atn_trace_shadow(atn_ctx* ctx, const atn_shadow_query* queries_host, uint32_t n, int32_t flavour, uint8_t* out_visible);
/* PathTracing::shade + ShadeMiss (renderer/pathtracing/pathtracing.cpp:91-236, pathtracing_impl.h:112-264, 353-509, 680-743,
 * pathtracing_nee_impl.h:23-95) for n caller-given vertices (atn_shade_vertex, aten_layout.h), through ONE launch of the PRODUCTION
 * shade kernel: a fill kernel writes each record into the context's own path buffers, in the slot its pixel owns, and a pattern no
 * kernel writes into every other slot, every plane a vertex does not read and both output queues; the live queue is handed over
 * shuffled (queue_order 0) or in the records' order (1); the launch goes through the renderer's own launcher, so it is the
 * instantiation atn_render picks for the uploaded scene's material set at the context's wave setting (ATEN_AMD_SHADE_WAVES), with the
 * chunk size of the launch plan or the forced one.  A check kernel then reads the results.
 * THE CONTRACT is what the next stages can observe (atn_shade_result): the flags, contrib, membership in the next bounce's queue and in
 * the shadow queue -- read from the queues the kernel appended to, not recomputed -- and, for a path that goes on, the next ray, pdf,
 * throughput and sampler dimension; for a path with a shadow ray, sh_o, sh_d and sh_c with their light bits.  What the reference
 * computes but nobody reads is NOT part of it: the shadow ray of a path that ended in this vertex, and the BSDF sample, throughput and
 * sampler position of a path that does not go on.  The kernel skips those on purpose; both this entry and its CPU twin report zeros.
 * Flavour 0 "plain" is k_shade<false, MS>.  Flavour 1 "svgf" is k_shade<true, MS> (SVGFRenderer::Shade, svgf/svgf.cpp:89-229): the
 * entry allocates three AOV planes of its own, a texel per pixel, and computes W2C from the camera as an SVGF frame does, so the context
 * needs no SVGF frame behind it; the result reports which of the three texels of its pixel the vertex wrote (aov_written) and their
 * values.  The look-ahead, deferred-NEE, regenerated and relaxed-math flavours are not served.
 * ATN_ERR_HIP with counts when an unused slot or AOV texel changed, a plane changed that a vertex leaves alone (hit record, accum,
 * done, the shadow record of a slot outside the shadow queue, the live queue, a queue entry behind its counter, a counter of another
 * depth), a slot is queued twice, or a queue holds a slot that was not handed in.
 * ATN_ERR_NO_SCENE without a scene; ATN_ERR_INVALID_ARG for null pointers, an unknown flavour or queue order, chunk_items > 4, a bounce
 * at or beyond max_depth, a pixel outside the frame, two records on one pixel, a terminated record, a hit record outside the scene;
 * ATN_ERR_UNSUPPORTED under atn_set_shade_math(1); n == 0 is a no-op. */
int atn_shade_stage(atn_ctx* ctx, const atn_shade_call* call, const atn_shade_vertex* records_host, uint32_t n, atn_shade_result* out_host);
/* n successive CMJ::nextSample() (src/libaten/sampler/cmj.h:32-37). */
int atn_cmj_samples(atn_ctx* ctx, uint32_t index, uint32_t dimension, uint32_t scramble, int32_t n, float* out_host);
/* For each of n (index, dimension, scramble) triples: CMJ::init then `draws` x nextSample()
 * (src/libaten/sampler/cmj.h:21-37); out_host[k * draws + d]. */
int atn_cmj_batch(atn_ctx* ctx, uint32_t n, const uint32_t* index, const uint32_t* dimension, const uint32_t* scramble,
                  int32_t draws, float* out_host);
/* ray::Offset (src/libaten/math/ray.h:26-74: "A Fast and Robust Method for Avoiding Self-Intersection", Ray Tracing Gems ch. 6)
 * as the kernels compute it for every next ray and shadow ray: n origins (xyz) and normals (xyz) -> n offset origins. */
/* The math-library functions the float path calls, evaluated by THIS build on the device (ocml sinf / cosf / atanf / acosf / atan2f /
 * logf / expf / powf, and the correctly rounded sqrtf, a / b, 1 / sqrtf): kind 0..10 in that order, b is the second argument where
 * there is one.  What the float tolerance of the parity contract is made of: tools/ulp_study.py holds these against the CPU build's
 * libm. */
int atn_libm_probe(atn_ctx* ctx, int32_t kind, uint32_t n, const float* a, const float* b, float* out_host);
int atn_ray_offset(atn_ctx* ctx, uint32_t n, const float* origins, const float* normals, float* out_host);
/* material::sampleMaterial / samplePDF / sampleBSDF tables (src/libaten/material/material_impl.h:24-206).
 * Case i samples with CMJ::init(index[i], dimension[i], scramble[i]) (dimension == NULL: 0 -- note that CMJ's pattern seed is
 * dimension * scramble, cmj.h:118-123, so the draw of dimension 0 ignores the scramble).
 * out_sample: n*7 {dir, bsdf, pdf}; out_eval: n*5 {samplePDF, sampleBSDF.bsdf, sampleBSDF.pdf} at wo = dir. */
int atn_material_table(atn_ctx* ctx, int32_t mtrl_id, uint32_t n, const float* nrm, const float* wi,
                       const uint32_t* index, const uint32_t* dimension, const uint32_t* scramble, const float* uv,
                       float* out_sample, float* out_eval);
/* material::samplePDF / sampleBSDF (material_impl.h:90-206) at caller-given outgoing directions wo (n * 3):
 * out_eval n*5 {samplePDF, sampleBSDF.bsdf.xyz, sampleBSDF.pdf}.  For invariants that need no oracle (the pdf integrates to
 * one, sampled directions follow it, bsdf * cos stays below one). */
int atn_material_eval(atn_ctx* ctx, int32_t mtrl_id, uint32_t n, const float* nrm, const float* wi, const float* wo,
                      const float* uv, float* out_eval);
/* Stable compaction of indices with flag > 0 (contract of idaten::StreamCompaction::compact,
 * src/libidaten/kernel/StreamCompaction.cu:175-316): the renderer's own queue append (one ballot + popcount
 * prefix per wave, one atomic per 1024-entry block chunk -- the call k_shade makes) followed by a host sort,
 * because the renderer's queues are unordered. */
int atn_compact(atn_ctx* ctx, const int32_t* flags_host, uint32_t n, int32_t* out_idx_host, uint32_t* out_count);
/* The queue append as the renderer uses it: two queues filled in one pass (entry i -> A when flags_a[i] > 0, -> B
 * when flags_b[i] > 0; flags_b may be NULL), outputs in the (racy) order the device produced.  grid_blocks = 0
 * picks the renderer's launch geometry; any other value forces that many 256-thread blocks (grid-stride path). */
int atn_compact2(atn_ctx* ctx, const int32_t* flags_a_host, const int32_t* flags_b_host, uint32_t n, uint32_t grid_blocks,
                 int32_t* out_a_host, uint32_t* out_count_a, int32_t* out_b_host, uint32_t* out_count_b);

/* ABI self-description for binding checks. */
uint32_t atn_sizeof_scene_desc(void);
uint32_t atn_sizeof_destination(void);
uint32_t atn_abi_version(void);         /* 3 (r04: atn_material_table's dimension argument, atn_compact3 dropped); 2 since atn_scene_desc carries the NPR fields */
/* "<sha16 of the kernel sources>|<extra compile flags>" of the loaded binary (the build recipe passes it in; "unknown" for a
 * hand-rolled build): profiling records name the build they were taken on. */
const char* atn_build_id(void);

#ifdef __cplusplus
}
#endif
#endif /* ATEN_AMD_H_ */
