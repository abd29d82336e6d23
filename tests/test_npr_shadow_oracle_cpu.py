"""The NPR shadow pre-pass on the CPU: the twin (tests/cxx/npr_shadow_oracle.cpp) -- its row filter against closed forms worked out
in float64, its pre-pass on scenedefs.stylized_shadow_room against what the scene is built to show -- and the library's new entry
points.  docs/NPR_SHADOW.md has the decisions."""
import os
import subprocess

import numpy as np
import pytest

import npr_shadow_oracle as S
from aten_amd import layout as L
from aten_amd.scene import scenedefs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("atn_npr_shadow_set_mode", "atn_npr_shadow_download", "atn_npr_shadow_filter")
W = H = 112
INF = np.float32(np.inf)


@pytest.fixture(scope="module")
def orc():
    from oracle import orc as o
    o.lib()
    return o


def test_library_exports_npr_shadow_entry_points():
    """The three atn_npr_shadow_* symbols: in the header, in the binding's list and in the built library's export table."""
    from aten_amd import _lib
    header = open(os.path.join(ROOT, "include", "aten_amd.h")).read()
    for s in SYMBOLS:
        assert "int %s(atn_ctx* ctx" % s in header, s
        assert s in _lib.SYMBOLS, s
    so = os.environ.get("ATEN_AMD_LIB") or os.path.join(ROOT, "aten_amd", "libaten_amd.so")
    out = subprocess.check_output(["nm", "-D", "--defined-only", so]).decode()
    names = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for s in SYMBOLS:
        assert s in names, s


# ---- the filter: w = exp(-(i*i)/8 - (dc - d)^2 / dc), 11 taps along the row, x clamped; clamp(den > 0 ? num / den : 1, 0, 1)
def g(i):
    return np.exp(-np.float64(i * i) / 8.0)


G_ALL = sum(g(i) for i in range(-5, 6))


def test_filter_all_lit_is_exactly_one():
    rng = np.random.default_rng(5)
    depth = rng.uniform(0.5, 9.0, (4, 37)).astype(np.float32)
    out = S.row_filter(np.ones_like(depth), depth)
    assert np.array_equal(out, np.ones_like(depth))     # numerator and denominator are the same sum


def test_filter_lit_step_at_uniform_depth():
    """lit = (x >= 20) at one depth: the sum of exp(-i^2 / 8) over the lit taps over the full sum."""
    w = 40
    lit = (np.arange(w) >= 20).astype(np.float32)[None, :]
    out = S.row_filter(lit, np.full((1, w), 3.25, np.float32))[0]
    for x in range(5, w - 5):
        want = sum(g(i) for i in range(-5, 6) if x + i >= 20) / G_ALL
        assert abs(float(out[x]) - want) <= 1e-6, (x, out[x], want)
    assert out[14] == 0.0 and out[25] == 1.0 and 0.0 < out[19] < 0.5 < out[20] < 1.0


@pytest.mark.parametrize("c,delta", [(2.0, 0.5), (4.0, 1.5), (1.0, 3.0)])
def test_filter_depth_step(c, delta):
    """Depth c left of x = 20 and c + delta from there on, lit only on the left: a tap across the step weighs exp(-delta^2 / centre
    depth) times its spatial weight -- the CENTRE's depth divides, so the two sides of the step see different weights."""
    w = 40
    x_all = np.arange(w)
    lit = (x_all < 20).astype(np.float32)[None, :]
    depth = np.where(x_all < 20, np.float32(c), np.float32(c) + np.float32(delta)).astype(np.float32)[None, :]
    out = S.row_filter(lit, depth)[0]
    d64 = np.float64(np.float32(c) + np.float32(delta)) - np.float64(np.float32(c))
    for x in range(5, w - 5):
        centre = np.float64(depth[0, x])
        across = np.exp(-d64 * d64 / centre)
        same = [g(i) for i in range(-5, 6) if (x + i < 20) == (x < 20)]
        other = [g(i) * across for i in range(-5, 6) if (x + i < 20) != (x < 20)]
        num = sum(same) if x < 20 else sum(other)
        want = num / (sum(same) + sum(other))
        assert abs(float(out[x]) - want) <= 1e-6, (x, out[x], want)


def test_filter_miss_centred_pixel_is_exactly_one():
    """A miss has depth +inf: centred on it every weight is NaN, the denominator is not > 0 and the result is exactly 1 -- whatever the
    neighbours hold; a hit next to a miss gives the miss weight 0."""
    lit = np.float32([[1, 0, 0, 0, 1, 1, 0, 0, 0, 0, 1, 1, 0]])
    depth = np.float32([[2, 2, INF, 2, 2, INF, INF, 2, 2, 2, 2, INF, 2]])
    out = S.row_filter(lit, depth)[0]
    assert np.all(out[np.isinf(depth[0])] == 1.0)
    x = 3       # taps x = 0..8 (i = -3..5, the two left ones replicate x = 0): misses weigh 0
    taps = [min(max(x + i, 0), 12) for i in range(-5, 6)]
    num = sum(g(i) for i, t in zip(range(-5, 6), taps) if np.isfinite(depth[0, t]) and lit[0, t] == 1)
    den = sum(g(i) for i, t in zip(range(-5, 6), taps) if np.isfinite(depth[0, t]))
    assert abs(float(out[x]) - num / den) <= 1e-6


@pytest.mark.parametrize("w", [13, 7, 1])
def test_filter_edges_and_narrow_rows(w):
    """x is clamped to the row: at the edges (and in rows narrower than the window: 7, 1) the border pixel is tapped repeatedly."""
    rng = np.random.default_rng(w)
    lit = (rng.uniform(size=(3, w)) < 0.5).astype(np.float32)
    depth = rng.uniform(1.0, 1.6, (3, w)).astype(np.float32)
    out = S.row_filter(lit, depth)
    for y in range(3):
        for x in range(w):
            c = np.float64(depth[y, x])
            num = den = 0.0
            for i in range(-5, 6):
                t = min(max(x + i, 0), w - 1)
                d = c - np.float64(depth[y, t])
                k = np.exp(-np.float64(i * i) / 8.0 - d * d / c)
                num += float(lit[y, t]) * k
                den += k
            assert abs(float(out[y, x]) - num / den) <= 1e-6, (y, x)
    if w == 1:
        assert np.array_equal(out, lit)      # eleven taps of the one pixel


# ---- the pre-pass on stylized_shadow_room
def _prepass(orc, scene, frame=0, w=W, h=H):
    fs, cam = scene
    c = orc.create_camera(cam["pos"], cam["at"], cam["vfov"], w, h)
    seeds = orc.init_sampler(w, h, 0)
    r = S.prepass(fs, c, seeds, w, h, frame=frame)
    hit = r["mtrl"] >= 0
    r["toon"] = hit & np.isin(fs.arrays["materials"]["type"][r["mtrl"].clip(0)], (L.MTRL_TOON, L.MTRL_STYLIZED))
    r["names"] = fs.names["materials"]
    return r


@pytest.mark.parametrize("frame", [0, 3])
def test_prepass_room(orc, frame):
    r = _prepass(orc, scenedefs.stylized_shadow_room(), frame)
    lit, depth, mtrl = r["lit"], r["depth"], r["mtrl"]
    assert set(np.unique(lit)) == {0.0, 1.0}
    hit = np.isfinite(depth)
    toon, plain = r["toon"], hit & ~r["toon"]
    # toon pixels lit and in the boxes' shadows; so the walls
    for px in (toon, plain):
        assert (lit[px] == 1).sum() > 100 and (lit[px] == 0).sum() > 100
    lamp = mtrl == r["names"].index("light")
    assert lamp.sum() > 30 and not lit[lamp].any()                  # an emissive first hit returns before FillShadowRay
    miss = ~hit
    assert miss.sum() > 500 and np.all(np.isposinf(depth[miss])) and not lit[miss].any() and np.array_equal(miss, mtrl < 0)
    assert np.all(r["plane"][miss] == 1.0)                          # NaN weights
    assert np.array_equal(r["plane"], S.row_filter(lit, depth))
    assert r["plane"].min() >= 0.0 and r["plane"].max() <= 1.0
    between = (r["plane"] > 0.0) & (r["plane"] < 1.0)
    assert between.sum() > 200                                      # shadow edges are soft along the row


def test_prepass_without_the_base_material_flag(orc):
    """enable_shadowray_base_stylized_shadow = 0: PathTracing::shade returns before FillShadowRay at a first-hit toon surface."""
    fs, cam = scenedefs.stylized_shadow_room()
    want = _prepass(orc, (fs, cam))
    fs.desc.enable_shadowray_base_stylized_shadow = 0
    r = _prepass(orc, (fs, cam))
    assert r["toon"].sum() > 2500 and not r["lit"][r["toon"]].any()
    assert np.array_equal(r["lit"][~r["toon"]], want["lit"][~want["toon"]])      # the walls keep their rays (and their draws)


def test_prepass_short_box_casts_its_shadow_on_the_floor(orc):
    """Without the short box 364 floor pixels (of the 1344 that show the floor in both rooms: outside the box's footprint in the
    image) turn from shadowed to lit, and none the other way.  (The count is held to >= 300: a libm that rounds a light sample
    another way moves single pixels on the shadow's edge.)"""
    a = _prepass(orc, scenedefs.stylized_shadow_room())
    b = _prepass(orc, scenedefs.stylized_shadow_room(short_box=False))
    fl = a["names"].index("floor")
    both = (a["mtrl"] == fl) & (b["mtrl"] == fl)
    assert both.sum() > 1000
    assert ((a["lit"] == 0) & (b["lit"] == 1) & both).sum() >= 300
    assert ((a["lit"] == 1) & (b["lit"] == 0) & both).sum() == 0


def test_prepass_looks_through_the_pane(orc):
    """The half-transparent pane under the lamp: with alpha blending on the shadow rays of the surfaces below are looked through it
    (up to 10 lookups) and reach the light; with it off one lookup ends on the pane and the ray counts as blocked."""
    fs, cam = scenedefs.stylized_shadow_room(alpha_blocker=True)
    on = _prepass(orc, (fs, cam))
    fs.desc.config.enable_alpha_blending = 0
    off = _prepass(orc, (fs, cam))
    bare = _prepass(orc, scenedefs.stylized_shadow_room())
    not_pane = on["mtrl"] != on["names"].index("pane")
    assert (~not_pane).sum() > 100
    through = (on["lit"] == 1) & (off["lit"] == 0) & not_pane
    assert through.sum() > 3000 and (through & on["toon"]).sum() > 500
    assert ((on["lit"] == 0) & (off["lit"] == 1)).sum() == 0
    # seen through, the pane changes nothing but the ray's restarts: the room without it is lit alike (ulp-close restarts aside)
    assert ((on["lit"] != bare["lit"]) & not_pane).sum() <= 5
