// CPU twin of the display tail (docs/TAA.md): the reference's TAA fragment shader (src/shader/taa_fs.glsl) and gamma shader
// (src/shader/gamma_fs.glsl) restated in plain C++ over float4 planes, row 0 at the bottom.  TEST INFRASTRUCTURE ONLY: compiled by
// tests/taa_oracle.py with -ffp-contract=off -fno-fast-math; the product never links it.
// Written independently of the device kernel (no LDS, no tiles: every tap reads its plane), with the same decisions (docs/TAA.md):
// clamp-to-edge for every read, GLSL's min / max / clamp / mix as comparisons, uv = (x + 0.5) / w, the bilinear expression order
// lerp(lerp(c00, c10, fx), lerp(c01, c11, fx), fy) with lerp(a, b, f) = (1 - f) a + f b, texel coordinates brought into [-1, n] before
// floor (NaN -> -1), one bit pattern for every stored NaN, a NaN quantising to 0.
#include <cmath>
#include <cstdint>
#include <cstring>

namespace {

struct V4 { float x, y, z, w; };
struct V3 { float x, y, z; };

inline float gmin(float x, float y) { return (y < x) ? y : x; }        // GLSL min
inline float gmax(float x, float y) { return (x < y) ? y : x; }        // GLSL max
inline float gclamp(float x, float lo, float hi) { return gmin(gmax(x, lo), hi); }
inline V4 min4(const V4& a, const V4& b) { return V4{ gmin(a.x, b.x), gmin(a.y, b.y), gmin(a.z, b.z), gmin(a.w, b.w) }; }
inline V4 max4(const V4& a, const V4& b) { return V4{ gmax(a.x, b.x), gmax(a.y, b.y), gmax(a.z, b.z), gmax(a.w, b.w) }; }
inline V4 avg4(const V4& a, const V4& b) { return V4{ 0.5f * (a.x + b.x), 0.5f * (a.y + b.y), 0.5f * (a.z + b.z), 0.5f * (a.w + b.w) }; }
inline int clampi(int v, int lo, int hi) { return (v < lo) ? lo : (hi < v) ? hi : v; }
inline float canon(float v)
{
    if (v != v) { const uint32_t q = 0x7fc00000u; std::memcpy(&v, &q, 4); }
    return v;
}

// taa_fs.glsl:40-49
inline V3 rgb2ycocg(float r, float g, float b)
{
    return V3{ r / 4.0f + g / 2.0f + b / 4.0f, r / 2.0f - b / 2.0f, -r / 4.0f + g / 2.0f - b / 4.0f };
}
// :66-70 + :109-120 without the fetch
inline V4 sample_color(const V4& c)
{
    const float lum = rgb2ycocg(c.x, c.y, c.z).x;
    const float d = 1.0f + lum;
    const V3 y = rgb2ycocg(c.x / d, c.y / d, c.z / d);
    return V4{ y.x, y.y, y.z, c.w };
}
inline const V4& texel(const V4* p, int w, int h, int x, int y) { return p[clampi(x, 0, w - 1) + clampi(y, 0, h - 1) * w]; }

inline void axis(float t, int n, int& i0, int& i1, float& f)
{
    t = (t >= -1.0f) ? t : -1.0f;
    t = (t > (float)n) ? (float)n : t;
    const float fl = std::floor(t);
    f = t - fl;
    const int i = (int)fl;
    i0 = clampi(i, 0, n - 1);
    i1 = clampi(i + 1, 0, n - 1);
}
inline V4 lerp4(const V4& a, const V4& b, float f)
{
    return V4{ (1.0f - f) * a.x + f * b.x, (1.0f - f) * a.y + f * b.y, (1.0f - f) * a.z + f * b.z, (1.0f - f) * a.w + f * b.w };
}
inline V4 history(const V4* hist, int w, int h, float u, float v)
{
    int x0, x1, y0, y1;
    float fx, fy;
    axis(u * (float)w - 0.5f, w, x0, x1, fx);
    axis(v * (float)h - 0.5f, h, y0, y1, fy);
    return lerp4(lerp4(hist[x0 + y0 * w], hist[x1 + y0 * w], fx), lerp4(hist[x0 + y1 * w], hist[x1 + y1 * w], fx), fy);
}
// :80-107
inline V3 clip_aabb(const V3& mn, const V3& mx, const V3& q)
{
    const V3 center{ 0.5f * (mx.x + mn.x), 0.5f * (mx.y + mn.y), 0.5f * (mx.z + mn.z) };
    const V3 half{ 0.5f * (mx.x - mn.x) + 0.00000001f, 0.5f * (mx.y - mn.y) + 0.00000001f, 0.5f * (mx.z - mn.z) + 0.00000001f };
    const V3 clip{ q.x - center.x, q.y - center.y, q.z - center.z };
    const V3 unit{ clip.x / half.x, clip.y / half.y, clip.z / half.z };
    const float ma = gmax(std::fabs(unit.x), gmax(std::fabs(unit.y), std::fabs(unit.z)));
    if (ma > 1.0f) return V3{ center.x + clip.x / ma, center.y + clip.y / ma, center.z + clip.z / ma };
    return q;
}
// this tap's velocity after the rescale of :205-208
inline void velocity(const V4& md, float& vx, float& vy, float& len2)
{
    vx = md.x; vy = md.y;
    len2 = (vx * vx + vy * vy) + 1e-6f;
    vx = vx / len2; vy = vy / len2;
    const float s = gmin(len2, 2.0f);
    vx = vx * s; vy = vy * s;
}
inline uint32_t unorm8(float g) { return (g >= 0.0f) ? (uint32_t)std::floor(g * 255.0f + 0.5f) : 0u; }
inline float gamma1(float c, float inv_gamma) { return canon(gclamp(std::pow(c, inv_gamma), 0.0f, 1.0f)); }

} // namespace

extern "C" {

// One frame.  cur / hist / motion / out / gamma_f: float4[w*h]; rgba8: uint32[w*h]; exp_args / weights (may be null): float[w*h][9],
// tap order y = -1..1 outer, x = -1..1 inner; NaN for a tap that was skipped and for every tap of a pixel that passed through.
void orc_taa_resolve(int w, int h, const float* cur_, const float* hist_, const float* motion_, int enable, float gamma,
                     float* out_, float* gamma_f_, uint32_t* rgba8, float* exp_args, float* weights)
{
    const V4* cur = reinterpret_cast<const V4*>(cur_);
    const V4* hist = reinterpret_cast<const V4*>(hist_);
    const V4* mot = reinterpret_cast<const V4*>(motion_);
    V4* out = reinterpret_cast<V4*>(out_);
    V4* gamma_f = reinterpret_cast<V4*>(gamma_f_);
    const float inv_gamma = 1.0f / gamma;
    const float qnan = std::nanf("");
    for (int iy = 0; iy < h; iy++)
        for (int ix = 0; ix < w; ix++) {
            const int idx = ix + iy * w;
            if (exp_args) for (int k = 0; k < 9; k++) exp_args[9 * idx + k] = qnan;
            if (weights) for (int k = 0; k < 9; k++) weights[9 * idx + k] = qnan;
            V4 o;
            if (!enable || !hist || mot[idx].z < 0.0f) {        // :136-149
                const V4 c = cur[idx];
                o = V4{ c.x, c.y, c.z, 1.0f };
            }
            else {
                V4 t[3][3];     // [row y - 1 .. y + 1][column x - 1 .. x + 1]: ctl ctc ctr / cml cmc cmr / cbl cbc cbr (:154-162)
                for (int y = -1; y <= 1; y++) for (int x = -1; x <= 1; x++) t[y + 1][x + 1] = sample_color(texel(cur, w, h, ix + x, iy + y));
                V4 cmin = min4(t[0][0], min4(t[0][1], min4(t[0][2], min4(t[1][0], min4(t[1][1], min4(t[1][2], min4(t[2][0], min4(t[2][1], t[2][2]))))))));
                V4 cmax = max4(t[0][0], max4(t[0][1], max4(t[0][2], max4(t[1][0], max4(t[1][1], max4(t[1][2], max4(t[2][0], max4(t[2][1], t[2][2]))))))));
                const V4 cmin5 = min4(t[0][1], min4(t[1][0], min4(t[1][1], min4(t[1][2], t[2][1]))));
                const V4 cmax5 = max4(t[0][1], max4(t[1][0], max4(t[1][1], max4(t[1][2], t[2][1]))));
                cmin = avg4(cmin, cmin5);
                cmax = avg4(cmax, cmax5);
                const V4 cc = t[1][1];
                const float u = ((float)ix + 0.5f) / (float)w, v = ((float)iy + 0.5f) / (float)h;
                float sx = 0.0f, sy = 0.0f, sz = 0.0f, weight = 0.0f;
                for (int y = -1; y <= 1; y++)
                    for (int x = -1; x <= 1; x++) {         // :184-247
                        const V4 md = texel(mot, w, h, ix + x, iy + y);
                        if (md.z < 0.0f) continue;
                        float vx, vy, len2;
                        velocity(md, vx, vy, len2);
                        const V4 nb4 = sample_color(history(hist, w, h, u + vx, v + vy));
                        const float len = std::sqrt(vx * vx + vy * vy);
                        const float arg = -2.29f * len * len;
                        float W = std::exp(arg);
                        W = W * (1.0f - gclamp(len2 / 2.0f, 0.0f, 1.0f));
                        const int k = (y + 1) * 3 + (x + 1);
                        if (exp_args) exp_args[9 * idx + k] = arg;
                        if (weights) weights[9 * idx + k] = W;
                        V3 nb = clip_aabb(V3{ cmin.x, cmin.y, cmin.z }, V3{ cmax.x, cmax.y, cmax.z }, V3{ nb4.x, nb4.y, nb4.z });
                        const float dx = std::fabs(nb.x - cc.x), dy = std::fabs(nb.y - cc.y), dz = std::fabs(nb.z - cc.z);
                        const float cl = std::sqrt(dy * dy + dz * dz);
                        if (0.32f < cl) {
                            const float s = 0.32f / cl;
                            nb = V3{ cc.x + s * dx, cc.y + s * dy, cc.z + s * dz };
                        }
                        sx = sx + nb.x * W; sy = sy + nb.y * W; sz = sz + nb.z * W;
                        weight = weight + W;
                    }
                if (weight > 0.0f) {        // :249-262
                    sx = sx / weight; sy = sy / weight; sz = sz / weight;
                    weight = weight / 9.0f;
                    const float mY = cc.x * (1.0f - weight) + sx * weight, mCo = cc.y * (1.0f - weight) + sy * weight, mCg = cc.z * (1.0f - weight) + sz * weight;
                    const float r = gclamp(mY + mCo - mCg, 0.0f, 1.0f), g = gclamp(mY + mCg, 0.0f, 1.0f), b = gclamp(mY - mCo - mCg, 0.0f, 1.0f);
                    const float d = 1.0f - rgb2ycocg(r, g, b).x;
                    o = V4{ r / d, g / d, b / d, 1.0f };
                }
                else o = cc;        // :263-265
            }
            o = V4{ canon(o.x), canon(o.y), canon(o.z), canon(o.w) };
            out[idx] = o;
            const float gr = gamma1(o.x, inv_gamma), gg = gamma1(o.y, inv_gamma), gb = gamma1(o.z, inv_gamma);
            if (gamma_f) gamma_f[idx] = V4{ gr, gg, gb, 1.0f };
            if (rgba8) rgba8[idx] = unorm8(gr) | (unorm8(gg) << 8) | (unorm8(gb) << 16) | 0xff000000u;
        }
}

// ---- helpers the tests hold to mathematics ----
void orc_taa_sample_color(const float* c, float* out) { const V4 r = sample_color(V4{ c[0], c[1], c[2], c[3] }); std::memcpy(out, &r, 16); }
void orc_taa_clip(const float* mn, const float* mx, const float* q, float* out)
{
    const V3 r = clip_aabb(V3{ mn[0], mn[1], mn[2] }, V3{ mx[0], mx[1], mx[2] }, V3{ q[0], q[1], q[2] });
    out[0] = r.x; out[1] = r.y; out[2] = r.z;
}
// the neighbourhood box of pixel (ix, iy): cmin[4], cmax[4]
void orc_taa_box(int w, int h, const float* cur_, int ix, int iy, float* cmin_, float* cmax_)
{
    const V4* cur = reinterpret_cast<const V4*>(cur_);
    V4 t[3][3];
    for (int y = -1; y <= 1; y++) for (int x = -1; x <= 1; x++) t[y + 1][x + 1] = sample_color(texel(cur, w, h, ix + x, iy + y));
    V4 cmin = t[2][2], cmax = t[2][2];
    const int order[8][2] = { {2, 1}, {2, 0}, {1, 2}, {1, 1}, {1, 0}, {0, 2}, {0, 1}, {0, 0} };
    for (const auto& o : order) { cmin = min4(t[o[0]][o[1]], cmin); cmax = max4(t[o[0]][o[1]], cmax); }
    const V4 cmin5 = min4(t[0][1], min4(t[1][0], min4(t[1][1], min4(t[1][2], t[2][1]))));
    const V4 cmax5 = max4(t[0][1], max4(t[1][0], max4(t[1][1], max4(t[1][2], t[2][1]))));
    cmin = avg4(cmin, cmin5); cmax = avg4(cmax, cmax5);
    std::memcpy(cmin_, &cmin, 16); std::memcpy(cmax_, &cmax, 16);
}
// the history tap of the pixel centre (ix, iy) for a motion/depth texel md: the raw bilinear fetch (out4) and where it was made (uv2)
void orc_taa_tap(int w, int h, const float* hist_, int ix, int iy, const float* md, float* out4, float* uv2)
{
    float vx, vy, len2;
    velocity(V4{ md[0], md[1], md[2], md[3] }, vx, vy, len2);
    const float u = ((float)ix + 0.5f) / (float)w + vx, v = ((float)iy + 0.5f) / (float)h + vy;
    const V4 r = history(reinterpret_cast<const V4*>(hist_), w, h, u, v);
    std::memcpy(out4, &r, 16);
    uv2[0] = u; uv2[1] = v;
}
void orc_taa_unorm8(const float* g, int n, uint32_t* out) { for (int i = 0; i < n; i++) out[i] = unorm8(gclamp(g[i], 0.0f, 1.0f)); }

} // extern "C"
