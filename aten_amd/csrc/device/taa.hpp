// The display tail behind SVGF / ReSTIR (docs/TAA.md): aten::TAA's fragment shader (src/shader/taa_fs.glsl) and aten::GammaCorrection's
// (src/shader/gamma_fs.glsl) as ONE launch per frame:
//   k_taa   per pixel: the current colour (s0), the history (s1) and the motion/depth plane (s2) -> the TAA output, which is also the
//           next frame's history (taa.cpp:33-60, the ping-pong), and behind it pow(rgb, 1 / gamma) as float4 (optional) and as RGBA8
// Every plane is float4[w*h], row 0 at the bottom.  A block of 256 covers svgf_pixel's 8 x 32 tile (svgf_frame.hpp) and stages the tile
// plus a one-texel halo (10 x 34 texels, coordinates clamped to the frame: fbo.cpp:78-79's GL_CLAMP taken as clamp-to-edge) in LDS once:
// the colour already through sampleColor (taa_fs.glsl:109-120: c / (1 + lum), then YCoCg), and what a tap needs of the texel's
// motion/depth: its rescaled velocity and its weight W (:205-219; they depend on the neighbour's texel alone, so they are computed per
// texel, 340 times a block, instead of per tap, 2304 times -- the same operations on the same operands).  The nine colour taps and
// nine motion taps read it from there; the up to nine bilinear history fetches go to global memory.
// LDS layout: three arrays -- the mapped colour (float4), the velocity (float2) and the weight (float; -1 where the depth is below 0) -- all with rows of kTaaPitch = 24
// elements; lane l of a wave reads element (l >> 3) * pitch + (l & 7) + a constant.  By the lane groups and bank rules of the LDS:
//   16- and 12-byte colour reads (the box's alpha is dead, so the compiler reads 12 of a texel's 16 bytes): groups of 16 (8) lanes made
//     of runs of four lanes from rows r, r + 1 or r + 2; the runs must fall on different 16-byte slots mod 16 (mod 8): pitch = 8 (mod 16)
//   8-byte velocity reads: 32 lanes = 4 rows of 8, 64 banks: the rows must start 16 dwords apart mod 64: 2 * pitch = 16 or 48 (mod 64)
//   4-byte weight reads: 32 lanes = 4 rows of 8, 32 banks: the rows must start 8 dwords apart mod 32: pitch = 8 or 24 (mod 32)
// The halo needs 10 elements per row; 24 is the smallest pitch that meets all three (10 itself is 2-way for every kind of read).
// The CPU tests enumerate the groups for every offset (docs/TAA.md).
// Arithmetic: one IEEE rounding per operation, no contraction, correctly rounded divide and square root (build.py); min / max / clamp /
// mix are GLSL's definitions written out as comparisons, so that a NaN takes the same way here and in the CPU twin
// (docs/TAA.md).  The only operations that are not bit-reproducible on the CPU are expf (the tap weight) and powf (gamma).
#pragma once
#include "svgf_frame.hpp"

namespace atn {

struct TaaArgs {
    const float4* cur;          // s0: the frame's colour
    const float4* hist;         // s1: the previous TAA output
    const float4* motion;       // s2: {prev - cur in screen fractions, depth (< 0: a miss), 1}
    float4* out;                // the TAA output = the next frame's history
    float4* gamma_f;            // pow(out.rgb, 1 / gamma) clamped to [0, 1], alpha 1 (null: not written)
    uint32_t* rgba8;            // the same as unorm8, R in the low byte
    int32_t width, height;
    int32_t enable;             // 0: the pass-through rule for every pixel (enableTAA off, and the first frame after a reset)
    float inv_gamma;            // 1.0F / gamma, rounded once on the host
};

constexpr int32_t kTaaTileW = 8, kTaaTileH = 32, kTaaHaloW = kTaaTileW + 2, kTaaHaloH = kTaaTileH + 2, kTaaPitch = 24;

// aten_amd.hip fills TaaArgs and calls the launcher (launch.hpp); the kernel is compiled in taa.hip only
#ifdef ATN_TAA_TU

struct taa3 { float x, y, z; };

// GLSL 4.20 section 8.3: min(x, y) = y < x ? y : x, max(x, y) = x < y ? y : x, clamp = min(max(x, lo), hi), mix = x * (1 - a) + y * a
ATN_DEV float taa_min(float x, float y) { return (y < x) ? y : x; }
ATN_DEV float taa_max(float x, float y) { return (x < y) ? y : x; }
ATN_DEV float taa_clamp(float x, float lo, float hi) { return taa_min(taa_max(x, lo), hi); }
ATN_DEV float4 taa_min4(const float4& a, const float4& b) { return make_float4(taa_min(a.x, b.x), taa_min(a.y, b.y), taa_min(a.z, b.z), taa_min(a.w, b.w)); }
ATN_DEV float4 taa_max4(const float4& a, const float4& b) { return make_float4(taa_max(a.x, b.x), taa_max(a.y, b.y), taa_max(a.z, b.z), taa_max(a.w, b.w)); }
// one bit pattern for every NaN the pass stores (the hardware's own default NaN and an x86 host's differ in the sign bit)
ATN_DEV float taa_canon(float v) { return (v != v) ? __uint_as_float(0x7fc00000u) : v; }

// RGB2YCoCg, taa_fs.glsl:40-49
ATN_DEV taa3 taa_rgb2ycocg(float r, float g, float b)
{
    return taa3{ r / 4.0F + g / 2.0F + b / 4.0F, r / 2.0F - b / 2.0F, -r / 4.0F + g / 2.0F - b / 4.0F };
}
// sampleColor without the fetch, taa_fs.glsl:66-70,109-120: map, then YCoCg; alpha passes through
ATN_DEV float4 taa_sample_color(const float4& c)
{
    const float lum = taa_rgb2ycocg(c.x, c.y, c.z).x;
    const float d = 1.0F + lum;
    const taa3 y = taa_rgb2ycocg(c.x / d, c.y / d, c.z / d);
    return make_float4(y.x, y.y, y.z, c.w);
}

// One axis of the bilinear history read: the texel coordinate t = u * n - 0.5 -> the two texel indices (clamp-to-edge) and the
// fraction.  t is first brought into [-1, n]: NaN and everything below -1 become -1, everything above n becomes n (outside that range
// both indices are the edge texel anyway), so floor, the fraction and the conversion to int32 never see a NaN, an inf or a value out
// of int32's range.
ATN_DEV void taa_axis(float t, int32_t n, int32_t& i0, int32_t& i1, float& f)
{
    t = (t >= -1.0F) ? t : -1.0F;
    t = (t > (float)n) ? (float)n : t;
    const float fl = floorf(t);
    f = t - fl;
    const int32_t i = (int32_t)fl;
    i0 = clampi(i, 0, n - 1);
    i1 = clampi(i + 1, 0, n - 1);
}
ATN_DEV float4 taa_lerp4(const float4& a, const float4& b, float f)      // lerp4 of shading.hpp: (1 - f) a + f b
{
    return make_float4((1.0F - f) * a.x + f * b.x, (1.0F - f) * a.y + f * b.y, (1.0F - f) * a.z + f * b.z, (1.0F - f) * a.w + f * b.w);
}
// texture2D(s1, uv) with GL_LINEAR and clamp-to-edge, in the expression order of sample_texture's bilinear branch (shading.hpp):
// lerp(lerp(c00, c10, fx), lerp(c01, c11, fx), fy)
ATN_DEV float4 taa_history(const float4* __restrict__ hist, int32_t w, int32_t h, float u, float v)
{
    int32_t x0, x1, y0, y1;
    float fx, fy;
    taa_axis(u * (float)w - 0.5F, w, x0, x1, fx);
    taa_axis(v * (float)h - 0.5F, h, y0, y1, fy);
    const float4 c00 = hist[x0 + y0 * w], c10 = hist[x1 + y0 * w], c01 = hist[x0 + y1 * w], c11 = hist[x1 + y1 * w];
    return taa_lerp4(taa_lerp4(c00, c10, fx), taa_lerp4(c01, c11, fx), fy);
}

// clipAABB, taa_fs.glsl:80-107
ATN_DEV taa3 taa_clip_aabb(const float4& mn, const float4& mx, const taa3& q)
{
    const taa3 center{ 0.5F * (mx.x + mn.x), 0.5F * (mx.y + mn.y), 0.5F * (mx.z + mn.z) };
    const taa3 half{ 0.5F * (mx.x - mn.x) + 0.00000001F, 0.5F * (mx.y - mn.y) + 0.00000001F, 0.5F * (mx.z - mn.z) + 0.00000001F };
    const taa3 clip{ q.x - center.x, q.y - center.y, q.z - center.z };
    const taa3 unit{ clip.x / half.x, clip.y / half.y, clip.z / half.z };
    const float ma = taa_max(fabsf(unit.x), taa_max(fabsf(unit.y), fabsf(unit.z)));
    if (ma > 1.0F) return taa3{ center.x + clip.x / ma, center.y + clip.y / ma, center.z + clip.z / ma };
    return q;
}

// gamma_fs.glsl:23-27 on one channel, and its unorm8 (round to nearest; a NaN quantises to 0)
ATN_DEV float taa_gamma(float c, float inv_gamma) { return taa_clamp(powf(c, inv_gamma), 0.0F, 1.0F); }
ATN_DEV uint32_t taa_unorm8(float g) { return (g >= 0.0F) ? (uint32_t)floorf(g * 255.0F + 0.5F) : 0u; }

__global__ void __launch_bounds__(256) k_taa(TaaArgs a)
{
    __shared__ float4 s_col[kTaaHaloH * kTaaPitch];
    __shared__ float2 s_mv[kTaaHaloH * kTaaPitch];
    __shared__ float s_w[kTaaHaloH * kTaaPitch];
    // svgf_pixel's block -> tile map (svgf_frame.hpp), kept whole-block: every thread of a tile inside the frame stages the halo
    const uint32_t gx = gridDim.x;
    const uint32_t b = blockIdx.x + blockIdx.y * gx;
    const uint32_t strip = gx >> 3;
    const uint32_t xcd = b & 7u, local = b >> 3;
    const int32_t x0 = (int32_t)((xcd * strip + local % strip) * (uint32_t)kTaaTileW), y0 = (int32_t)((local / strip) * (uint32_t)kTaaTileH);
    const int32_t w = a.width, h = a.height;
    if (x0 >= w || y0 >= h) return;     // (the whole block: uniform)
    const int32_t tx = (int32_t)(threadIdx.x & 7u), ty = (int32_t)(threadIdx.x >> 3);
    const int32_t ix = x0 + tx, iy = y0 + ty;
    if (a.enable) {
        for (int32_t i = (int32_t)threadIdx.x; i < kTaaHaloW * kTaaHaloH; i += 256) {
            const int32_t hx = i % kTaaHaloW, hy = i / kTaaHaloW;
            const int32_t g = clampi(x0 - 1 + hx, 0, w - 1) + clampi(y0 - 1 + hy, 0, h - 1) * w;
            s_col[hy * kTaaPitch + hx] = taa_sample_color(a.cur[g]);
            const float4 md = a.motion[g];
            // :203-208, :216-219.  W is never negative (exp >= 0, 1 - clamp(., 0, 1) >= 0; a NaN stays a NaN and counts, as in the shader)
            float vx = md.x, vy = md.y;
            const float len2 = (vx * vx + vy * vy) + 1e-6F;
            vx = vx / len2; vy = vy / len2;
            const float s = taa_min(len2, 2.0F);
            vx = vx * s; vy = vy * s;
            const float len = sqrtf(vx * vx + vy * vy);
            float W = expf(-2.29F * len * len);
            W = W * (1.0F - taa_clamp(len2 / 2.0F, 0.0F, 1.0F));
            s_mv[hy * kTaaPitch + hx] = make_float2(vx, vy);
            s_w[hy * kTaaPitch + hx] = (md.z < 0.0F) ? -1.0F : W;
        }
        __syncthreads();
    }
    if (ix >= w || iy >= h) return;
    const int32_t idx = ix + iy * w;
    const int32_t lc = (ty + 1) * kTaaPitch + tx + 1;
    float4 o;
    // taa_fs.glsl:136-149: TAA off, or no surface under the pixel centre: the current texel, alpha 1
    if (!a.enable || s_w[lc] < 0.0F) {
        const float4 c = a.cur[idx];
        o = make_float4(c.x, c.y, c.z, 1.0F);
    }
    else {
        // :154-173 ("t" is the row below: gl_FragCoord's y grows upwards and the taps are uv - dv)
        const float4 ctl = s_col[lc - kTaaPitch - 1], ctc = s_col[lc - kTaaPitch], ctr = s_col[lc - kTaaPitch + 1];
        const float4 cml = s_col[lc - 1], cmc = s_col[lc], cmr = s_col[lc + 1];
        const float4 cbl = s_col[lc + kTaaPitch - 1], cbc = s_col[lc + kTaaPitch], cbr = s_col[lc + kTaaPitch + 1];
        float4 cmin = taa_min4(ctl, taa_min4(ctc, taa_min4(ctr, taa_min4(cml, taa_min4(cmc, taa_min4(cmr, taa_min4(cbl, taa_min4(cbc, cbr))))))));
        float4 cmax = taa_max4(ctl, taa_max4(ctc, taa_max4(ctr, taa_max4(cml, taa_max4(cmc, taa_max4(cmr, taa_max4(cbl, taa_max4(cbc, cbr))))))));
        const float4 cmin5 = taa_min4(ctc, taa_min4(cml, taa_min4(cmc, taa_min4(cmr, cbc))));
        const float4 cmax5 = taa_max4(ctc, taa_max4(cml, taa_max4(cmc, taa_max4(cmr, cbc))));
        cmin = make_float4(0.5F * (cmin.x + cmin5.x), 0.5F * (cmin.y + cmin5.y), 0.5F * (cmin.z + cmin5.z), 0.5F * (cmin.w + cmin5.w));
        cmax = make_float4(0.5F * (cmax.x + cmax5.x), 0.5F * (cmax.y + cmax5.y), 0.5F * (cmax.z + cmax5.z), 0.5F * (cmax.w + cmax5.w));
        // (cavg is computed by the shader and never used)
        const float4 cc = cmc;
        const float u = ((float)ix + 0.5F) / (float)w, v = ((float)iy + 0.5F) / (float)h;
        float sx = 0.0F, sy = 0.0F, sz = 0.0F, weight = 0.0F;
        // :184-247
        for (int32_t y = -1; y <= 1; y++)
            for (int32_t x = -1; x <= 1; x++) {
                const float W = s_w[lc + y * kTaaPitch + x];
                if (W < 0.0F) continue;         // the neighbour's depth is below 0 (:199-201)
                const float2 mv = s_mv[lc + y * kTaaPitch + x];
                // the history is read at the CENTRE's uv + this tap's velocity (:210)
                const float4 nb4 = taa_sample_color(taa_history(a.hist, w, h, u + mv.x, v + mv.y));
                taa3 nb = taa_clip_aabb(cmin, cmax, taa3{ nb4.x, nb4.y, nb4.z });
                const float dx = fabsf(nb.x - cc.x), dy = fabsf(nb.y - cc.y), dz = fabsf(nb.z - cc.z);
                const float cl = sqrtf(dy * dy + dz * dz);
                if (0.32F < cl) {
                    // :235-238: the ABSOLUTE difference, scaled, is added to the centre
                    const float k = 0.32F / cl;
                    nb = taa3{ cc.x + k * dx, cc.y + k * dy, cc.z + k * dz };
                }
                sx = sx + nb.x * W; sy = sy + nb.y * W; sz = sz + nb.z * W;
                weight = weight + W;
            }
        // :249-265
        if (weight > 0.0F) {
            sx = sx / weight; sy = sy / weight; sz = sz / weight;
            weight = weight / 9.0F;
            const float mY = cc.x * (1.0F - weight) + sx * weight, mCo = cc.y * (1.0F - weight) + sy * weight, mCg = cc.z * (1.0F - weight) + sz * weight;
            // YCoCg2RGB (:51-62) clamps to [0, 1]; unmap (:72-76) divides by 1 - lum, which is 0 for a saturated colour: inf stays
            const float r = taa_clamp(mY + mCo - mCg, 0.0F, 1.0F), g = taa_clamp(mY + mCg, 0.0F, 1.0F), bl = taa_clamp(mY - mCo - mCg, 0.0F, 1.0F);
            const float d = 1.0F - taa_rgb2ycocg(r, g, bl).x;
            o = make_float4(r / d, g / d, bl / d, 1.0F);
        }
        else o = cc;        // :263-265: no tap counted: the centre as sampleColor left it (mapped, YCoCg), the source's alpha
    }
    o = make_float4(taa_canon(o.x), taa_canon(o.y), taa_canon(o.z), taa_canon(o.w));
    a.out[idx] = o;
    const float gr = taa_canon(taa_gamma(o.x, a.inv_gamma)), gg = taa_canon(taa_gamma(o.y, a.inv_gamma)), gb = taa_canon(taa_gamma(o.z, a.inv_gamma));
    if (a.gamma_f) a.gamma_f[idx] = make_float4(gr, gg, gb, 1.0F);
    a.rgba8[idx] = taa_unorm8(gr) | (taa_unorm8(gg) << 8) | (taa_unorm8(gb) << 16) | 0xff000000u;
}

#endif  // ATN_TAA_TU

} // namespace atn
