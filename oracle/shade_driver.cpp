/* TEST INFRASTRUCTURE.  A stand-alone program over the oracle's shade-stage entries, so that they can run under
 * -fsanitize=address,undefined without an interpreter around them (`make -C oracle shade_driver_san OUT=...`): the oracle's own
 * translation unit is compiled INTO this program.  It reads a scene blob -- the flat arrays behind an atn_scene_desc, written by
 * tests/test_shade_stage_cpu.py from the scene the Python builder assembled --, runs orc_record_vertices over one frame, then
 * orc_shade_stage on every bounce's records, and checks that each bounce's outputs are the next bounce's recorded inputs bit for bit.
 *
 * blob: uint32 magic 'ATNS', width, height, max_depth, rr_depth, n_objects, n_matrices, n_materials, n_lights, n_triangles,
 *       n_vertices, n_bvh_lists, n_textures, n_seeds; then uint32 count per BVH list; then int32 {width, height} per texture; then
 *       atn_scene_rendering_config, bbox min[3] max[3], atn_camera_param, and the arrays in the order of the counts (vtx_pos, vtx_nml
 *       for the vertices; the node lists; the textures' texels; the seeds).
 *       NOT carried: the NPR target lights, the screen-space texture and enable_shadowray_base_stylized_shadow (set to 1, the
 *       builder's default) -- a toon scene would need those fields in the blob.
 * usage: shade_driver scene.blob      exit status 0 = every check held. */
#include "aten_oracle.cpp"

#include <fstream>

namespace {
struct Reader {
    std::vector<char> buf; size_t at = 0; bool ok = true;
    template <class T> void get(T* dst, size_t n)
    {
        const size_t bytes = n * sizeof(T);
        if (!ok || at + bytes > buf.size()) { ok = false; return; }
        if (bytes) std::memcpy(dst, buf.data() + at, bytes);
        at += bytes;
    }
    template <class T> std::vector<T> vec(size_t n) { std::vector<T> v(n); get(v.data(), n); return v; }
};
}

int main(int argc, char** argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: shade_driver scene.blob\n"); return 2; }
    Reader rd;
    {
        std::ifstream f(argv[1], std::ios::binary);
        rd.buf.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
    }
    uint32_t h[14] = {};
    rd.get(h, 14);
    if (!rd.ok || h[0] != 0x534e5441u) { std::fprintf(stderr, "not a scene blob\n"); return 2; }
    const int32_t width = (int32_t)h[1], height = (int32_t)h[2], max_depth = (int32_t)h[3], rr_depth = (int32_t)h[4];
    const uint32_t n_lists = h[11], n_tex = h[12], n_seeds = h[13];
    std::vector<uint32_t> list_counts = rd.vec<uint32_t>(n_lists);
    std::vector<int32_t> tex_sizes = rd.vec<int32_t>((size_t)2 * n_tex);
    atn_scene_desc d{};
    rd.get(&d.config, 1); rd.get(d.scene_bbox_min, 3); rd.get(d.scene_bbox_max, 3);
    atn_camera_param cam{};
    rd.get(&cam, 1);
    auto objects = rd.vec<atn_object_param>(h[5]); auto matrices = rd.vec<atn_mat4>(h[6]); auto materials = rd.vec<atn_material_param>(h[7]);
    auto lights = rd.vec<atn_light_param>(h[8]); auto triangles = rd.vec<atn_triangle_param>(h[9]);
    auto pos = rd.vec<atn_vec4>(h[10]); auto nml = rd.vec<atn_vec4>(h[10]);
    std::vector<std::vector<atn_bvh_node>> nodes; std::vector<atn_bvh_list> lists(n_lists);
    for (uint32_t k = 0; k < n_lists; k++) { nodes.push_back(rd.vec<atn_bvh_node>(list_counts[k])); lists[k].nodes = nodes[k].data(); lists[k].count = list_counts[k]; }
    std::vector<std::vector<atn_vec4>> texels; std::vector<atn_texture_desc> tex(n_tex);
    for (uint32_t k = 0; k < n_tex; k++) {
        texels.push_back(rd.vec<atn_vec4>((size_t)tex_sizes[2 * k] * tex_sizes[2 * k + 1]));
        tex[k].texels = texels[k].data(); tex[k].width = tex_sizes[2 * k]; tex[k].height = tex_sizes[2 * k + 1];
    }
    auto seeds = rd.vec<uint32_t>(n_seeds);
    if (!rd.ok || rd.at != rd.buf.size()) { std::fprintf(stderr, "scene blob: wrong size\n"); return 2; }
    d.objects = objects.data(); d.n_objects = h[5]; d.matrices = matrices.data(); d.n_matrices = h[6];
    d.materials = materials.data(); d.n_materials = h[7]; d.lights = lights.data(); d.n_lights = h[8];
    d.triangles = triangles.data(); d.n_triangles = h[9]; d.vtx_pos = pos.data(); d.vtx_nml = nml.data(); d.n_vertices = h[10];
    d.bvh_lists = lists.data(); d.n_bvh_lists = n_lists; d.textures = tex.data(); d.n_textures = n_tex;
    d.enable_shadowray_base_stylized_shadow = 1;

    orc_destination dst{}; dst.width = width; dst.height = height; dst.maxDepth = max_depth; dst.russianRouletteDepth = rr_depth; dst.sample = 1;
    const uint64_t cap = (uint64_t)width * height * max_depth;
    std::vector<atn_shade_vertex> rec(cap); std::vector<int32_t> bounce(cap); std::vector<atn_vec4> contrib((size_t)width * height);
    const int64_t m = orc_record_vertices(&d, &cam, seeds.data(), n_seeds, &dst, 0, rec.data(), bounce.data(), cap, contrib.data());
    if (m <= 0) { std::fprintf(stderr, "orc_record_vertices returned %lld\n", (long long)m); return 1; }
    if (orc_record_vertices(&d, &cam, seeds.data(), n_seeds, &dst, 0, rec.data(), bounce.data(), 1, nullptr) != -1) { std::fprintf(stderr, "a short buffer was accepted\n"); return 1; }

    int failures = 0;
    std::vector<atn_shade_vertex> prev_in; std::vector<atn_shade_result> prev_out;
    for (int32_t b = 0; b < max_depth; b++) {
        std::vector<atn_shade_vertex> in;
        for (int64_t i = 0; i < m; i++) if (bounce[i] == b) in.push_back(rec[i]);
        std::vector<atn_shade_result> out(in.size()); std::vector<uint32_t> cat(in.size()); std::vector<float> margins(2 * in.size());
        atn_shade_call call{}; call.width = width; call.height = height; call.bounce = b; call.max_depth = max_depth; call.rr_depth = rr_depth;
        const int rc = orc_shade_stage(&d, &cam, seeds.data(), n_seeds, &call, in.data(), (uint32_t)in.size(), out.data(), cat.data(), margins.data());
        if (rc != 0) { std::fprintf(stderr, "orc_shade_stage(bounce %d) returned %d\n", b, rc); return 1; }
        {       // the same records through the "svgf" flavour: at bounce 0 every vertex writes its normal / depth and albedo / id texels
            std::vector<atn_shade_result> sv(in.size());
            call.flavour = 1;
            if (orc_shade_stage(&d, &cam, seeds.data(), n_seeds, &call, in.data(), (uint32_t)in.size(), sv.data(), nullptr, nullptr) != 0) failures++;
            for (size_t i = 0; i < sv.size(); i++) if (b == 0 ? (sv[i].aov_written & 3u) != 3u : (sv[i].aov_written & 4u) != 0u) { failures++; break; }
        }
        if (b > 0) {        // the previous bounce's outputs that go on ARE this bounce's inputs, in order, bit for bit
            size_t k = 0;
            for (size_t i = 0; i < prev_out.size(); i++) {
                if (!prev_out[i].goes_on) continue;
                if (k >= in.size()) { failures++; break; }
                const atn_shade_result& o = prev_out[i]; const atn_shade_vertex& v = in[k++];
                if (prev_in[i].pixel != v.pixel || std::memcmp(o.org, v.org, 12) || std::memcmp(o.dir, v.dir, 12) || std::memcmp(&o.pdfb, &v.pdfb, 4)
                    || std::memcmp(o.throughput, v.throughput, 12) || o.dimension != v.dimension || (o.flags & ~kFlagHit) != v.flags) failures++;
            }
            if (k != in.size()) failures++;
        }
        std::printf("bounce %d: %zu vertices\n", b, in.size());
        prev_in.swap(in); prev_out.swap(out);
    }
    // the refusals index nothing: a pixel, an object and a triangle outside their arrays, a terminated record
    if (!prev_in.empty()) {
        atn_shade_call call{}; call.width = width; call.height = height; call.bounce = max_depth - 1; call.max_depth = max_depth; call.rr_depth = rr_depth;
        atn_shade_result o{};
        for (int k = 0; k < 4; k++) {
            atn_shade_vertex v = prev_in[0];
            if (k == 0) v.pixel = width * height; else if (k == 1) { v.objid = (int32_t)d.n_objects; v.tri_id = 0; }
            else if (k == 2) { v.objid = 0; v.tri_id = (int32_t)d.n_triangles; } else v.flags |= kFlagTerminated;
            if (orc_shade_stage(&d, &cam, seeds.data(), n_seeds, &call, &v, 1, &o, nullptr, nullptr) != -1) failures++;
        }
    }
    if (failures) { std::fprintf(stderr, "%d checks failed\n", failures); return 1; }
    std::printf("ok: %lld vertices\n", (long long)m);
    return 0;
}
