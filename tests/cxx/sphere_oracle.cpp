/*
 * TEST INFRASTRUCTURE ONLY -- the CPU twin of atn_set_sphere_intersection(1) (docs/SPHERES.md).
 *
 * oracle/orc_core.h's TraverseClosest is aten::ThreadedBvhTraverser, which never tests a sphere.  TraverseClosestSpheres
 * below is that walk plus the leaf step of the reference's stackless walk for a top-layer leaf without a nested tree: sphere::hit
 * (orc_core.h: sphere_hit, quirks included) on the WORLD ray against isect_tmp.t = INF, the triangle leaf's acceptance, the hit
 * carrying sphere.mtrl_id.  orc_pt.h's frame loop and HitTestToTargetLight call TraverseClosest unqualified: the macro below makes
 * them -- and nothing in oracle/ -- use the twin's walk.  With no such leaf in the scene every result is the oracle's.
 */
#include "../../oracle/orc_core.h"

namespace orc {

inline bool TraverseClosestSpheres(Isect& isect, const Scene& ctxt, const Ray r, float t_min, float t_max,
    TraverseStats* stats = nullptr)
{
    t_min = ctxt.cfg().bvh_hit_min > 0 ? ctxt.cfg().bvh_hit_min : t_min;
    isect.isVoxel = false;

    const atn_bvh_node* node_list = ctxt.GetBvhNodes(0);
    Ray transformed_ray = r;
    int32_t nodeid = 0;
    int32_t objid = -1, meshid = -1;
    int32_t top_layer_hit = -1, top_layer_miss = -1;
    bool in_top = true;

    while (nodeid >= 0) {
        bool is_hit = false;
        atn_bvh_node node = node_list[nodeid];
        if (stats) stats->nodes++;

        if (node.f0 >= 0 || node.f1 >= 0) {
            if (node.f2 >= 0) {
                const auto& obj = ctxt.GetObject(static_cast<uint32_t>(node.f0));
                if (obj.mtx_id >= 0) {
                    const m4 mtx_W2L = ctxt.GetMatrix(obj.mtx_id + 1);
                    transformed_ray = Ray(mtx_W2L.apply(r.org), mtx_W2L.applyXYZ(r.dir));
                }
                else {
                    transformed_ray = r;
                }
                uint32_t bits = (uint32_t)float_as_int(node.f2);
                int32_t exid = ATN_EXID_MAIN(bits);
                node_list = ctxt.GetBvhNodes(exid);
                objid = static_cast<int32_t>(node.f0);
                meshid = static_cast<int32_t>(node.f3);
                top_layer_hit = static_cast<int32_t>(node.hit);
                top_layer_miss = static_cast<int32_t>(node.miss);
                is_hit = true;
                node.hit = 0;
                in_top = false;
            }
            else if (node.f1 >= 0) {
                const auto& prim = ctxt.GetTriangle(static_cast<uint32_t>(node.f1));
                Isect isect_tmp;
                isect_tmp.t = INF;
                if (stats) stats->tris++;
                is_hit = triangle_hit(prim, ctxt, transformed_ray, &isect_tmp);
                bool is_intersect = t_min < isect_tmp.t && (is_hit && isect_tmp.t < isect.t);
                if (is_intersect) {
                    isect = isect_tmp;
                    isect.objid = objid;
                    isect.tri_id = static_cast<int32_t>(node.f1);
                    isect.mtrlid = static_cast<int32_t>(prim.mtrlid);
                    isect.meshid = static_cast<int32_t>(prim.mesh_id);
                    isect.meshid = (isect.meshid < 0 ? meshid : isect.meshid);
                    t_max = isect.t;
                }
            }
            else if (in_top && ctxt.GetObject(static_cast<uint32_t>(node.f0)).type == ATN_OBJ_SPHERE) {
                // the sphere leaf's step: the triangle leaf's with sphere::hit as the primitive test, on the world ray
                const auto& obj = ctxt.GetObject(static_cast<uint32_t>(node.f0));
                Isect isect_tmp;
                isect_tmp.t = INF;
                is_hit = sphere_hit(obj, r, t_min, t_max, &isect_tmp);
                bool is_intersect = t_min < isect_tmp.t && (is_hit && isect_tmp.t < isect.t);
                if (is_intersect) {
                    isect = isect_tmp;
                    isect.objid = static_cast<int32_t>(node.f0);
                    isect.tri_id = -1;
                    isect.mtrlid = obj.sphere.mtrl_id;
                    isect.meshid = static_cast<int32_t>(node.f3);
                    isect.a = isect.t; isect.b = 0.0F;      // what the device's hit record carries: shade needs t
                    t_max = isect.t;
                }
            }
        }
        else {
            is_hit = aabb_hit(transformed_ray, ld3(node.boxmin), ld3(node.boxmax), t_min, t_max);
        }

        nodeid = static_cast<int32_t>(is_hit ? node.hit : node.miss);

        if (nodeid < 0) {
            nodeid = is_hit ? top_layer_hit : top_layer_miss;
            top_layer_hit = -1;
            top_layer_miss = -1;
            node_list = ctxt.GetBvhNodes(0);
            transformed_ray = r;
            in_top = true;
        }
    }
    return (isect.objid >= 0);
}

} // namespace orc

#define TraverseClosest TraverseClosestSpheres
#include "../../oracle/orc_pt.h"
#undef TraverseClosest
#include <omp.h>

using namespace orc;

extern "C" {

// per ray: the closest hit of the twin's walk (t, objid, tri, a, b in atn_intersection)
void sorc_trace_closest(const atn_scene_desc* scene, const atn_ray* rays, uint32_t n, float t_min, float t_max, atn_intersection* out)
{
    Scene ctxt(scene);
#pragma omp parallel for
    for (int64_t i = 0; i < (int64_t)n; i++) {
        Ray r; r.org = ld3(rays[i].org); r.dir = ld3(rays[i].dir);
        Isect is;
        TraverseClosestSpheres(is, ctxt, r, t_min, t_max, nullptr);
        atn_intersection& o = out[i];
        o.t = is.t; o.objid = is.objid; o.mtrlid = is.mtrlid; o.meshid = is.meshid;
        o.tri_id = is.tri_id; o.a = is.a; o.b = is.b; o.isVoxel = is.isVoxel;
    }
}

// per query: HitTestToTargetLight's verdict over the twin's walk, the ray re-normalised as HitShadowRay does
void sorc_shadow_visible(const atn_scene_desc* scene, const atn_shadow_query* q, uint32_t n, uint8_t* visible)
{
    Scene ctxt(scene);
#pragma omp parallel for
    for (int64_t i = 0; i < (int64_t)n; i++) {
        const Ray original_ray(ld3(q[i].org), ld3(q[i].dir));
        visible[i] = HitTestToTargetLight(ctxt, original_ray, ctxt.GetLight(q[i].light), q[i].dist_to_light, (q[i].flags & 1u) ? 1 : 0, nullptr, nullptr) ? 1 : 0;
    }
}

// one frame of aten::PathTracing::render over the twin's walk: orc_render's signature (oracle/aten_oracle.cpp: orc_render_cost without
// the cost map), progressive film or overwrite
struct sorc_destination { int32_t width, height, maxDepth, russianRouletteDepth, sample; uint32_t frame; int32_t progressive, nthreads; };
void sorc_render(const atn_scene_desc* scene, const atn_camera_param* camera, const uint32_t* seeds, uint32_t n_seeds,
    const sorc_destination* dst, atn_vec4* film, uint64_t* counters_out)
{
    (void)counters_out;
    Scene ctxt(scene);
    const int32_t width = dst->width, height = dst->height;
    const uint32_t samples = (uint32_t)dst->sample;
    int32_t maxDepth = dst->maxDepth;
    int32_t rrDepth = dst->russianRouletteDepth;
    if (rrDepth > maxDepth) rrDepth = maxDepth - 1;     // pathtracing.cpp:282-284
    if (dst->nthreads > 0) omp_set_num_threads(dst->nthreads);
#pragma omp parallel for
    for (int32_t y = 0; y < height; y++) {
        for (int32_t x = 0; x < width; x++) {
            v3 col(0); uint32_t cnt = 0;
            int32_t idx = y * width + x;
            PathState path;
            path.samples = 0;
            Ray ray; ShadowRay shadow_ray;
            for (uint32_t i = 0; i < samples; i++) {
                const uint32_t rnd = seeds[idx % n_seeds];
                GeneratePath(ray, x, y, (int32_t)i, dst->frame, path, *camera, rnd);
                path.contrib = v3(0);
                radiance(path, ray, shadow_ray, x, y, width, height, ctxt, *camera, maxDepth, rrDepth, nullptr);
                if (isInvalidColor(path.contrib)) continue;
                col += path.contrib;
                cnt++;
                if (path.is_terminated) break;
            }
            col /= (float)cnt;
            v4 v(col, 1);
            atn_vec4& cur = film[idx];
            if (dst->progressive) {
                float n = static_cast<float>(static_cast<int32_t>(cur.w));
                v4 c(cur.x, cur.y, cur.z, cur.w);
                c = n * c + v;
                float d = n + 1;
                cur.x = c.x / d; cur.y = c.y / d; cur.z = c.z / d;
                cur.w = n + 1;
            }
            else {
                cur.x = v.x; cur.y = v.y; cur.z = v.z; cur.w = v.w;
            }
        }
    }
}

}
