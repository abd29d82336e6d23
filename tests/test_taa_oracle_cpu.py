"""The CPU twin of the display tail (tests/cxx/taa_oracle.cpp; docs/TAA.md) held to mathematics, the library's exports, and the
kernel's LDS layout by the bank rule.  No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

import taa_oracle as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAA_SYMBOLS = ("atn_taa_resolve", "atn_taa_upload", "atn_taa_download", "atn_taa_reset")
F = np.float32


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def still(h, w, depth=1.0):
    m = np.zeros((h, w, 4), np.float32)
    m[..., 2] = depth
    m[..., 3] = 1.0
    return m


def test_library_exports_taa_entry_points():
    """The atn_taa_* symbols: in the header, in the binding's list and in the built library's export table; atn_mgpu_* has no form."""
    from aten_amd import _lib
    header = open(os.path.join(ROOT, "include", "aten_amd.h")).read()
    for s in TAA_SYMBOLS:
        assert "int %s(atn_ctx* ctx" % s in header, s
        assert s in _lib.SYMBOLS, s
    assert "void* atn_taa_output_device(atn_ctx* ctx)" in header and "atn_taa_output_device" in _lib.SYMBOLS
    so = os.environ.get("ATEN_AMD_LIB") or os.path.join(ROOT, "aten_amd", "libaten_amd.so")
    out = subprocess.check_output(["nm", "-D", "--defined-only", so]).decode()
    names = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for s in TAA_SYMBOLS + ("atn_taa_output_device",):
        assert s in names, s
    assert not [n for n in names if n.startswith("atn_mgpu_taa")]


def test_constant_frame_is_a_fixed_point_up_to_the_round_trip():
    """Zero motion, history = colour = one value per frame: every tap fetches that value, the box is a point, and the output is the
    input through map -> YCoCg -> mix -> RGB -> unmap.  Bound: about twenty roundings of values <= 1 (the divisions by 2 and 4 are
    exact), each 2^-24 absolute, and unmap divides by 1 - lum' with lum' = lum / (1 + lum) <= 1/2 for colours in [0, 1], which at
    most doubles them: 64 * 2^-24 absolute is three times that."""
    rng = np.random.default_rng(5)
    for _ in range(24):
        c = rng.random(4, np.float32)
        cur = np.broadcast_to(c, (5, 6, 4)).copy()
        out, gf, g8 = T.resolve(cur, cur, still(5, 6))
        assert np.all(out[..., 3] == 1.0)
        assert np.max(np.abs(out[..., :3] - c[:3])) <= 64 * 2.0 ** -24, (c, out[0, 0])


def test_disabled_or_missed_passes_the_texel_through():
    rng = np.random.default_rng(6)
    cur = (rng.random((7, 9, 4), np.float32) * F(8)).astype(np.float32)
    hist = (rng.random((7, 9, 4), np.float32) * F(8)).astype(np.float32)
    mot = still(7, 9)
    mot[..., :2] = (rng.random((7, 9, 2), np.float32) - F(0.5)) * F(0.2)
    want = cur.copy()
    want[..., 3] = 1.0
    out = T.resolve(cur, hist, mot, enable=False)[0]
    assert np.array_equal(bits(out), bits(want))
    out = T.resolve(cur, None, mot, enable=True)[0]        # no history: the first-frame rule
    assert np.array_equal(bits(out), bits(want))
    miss = rng.random((7, 9)) < 0.4
    miss[3, :] = True
    mot[miss, 2] = -1.0
    out, _, _, ea, ws = T.resolve(cur, hist, mot, enable=True, extras=True)
    assert np.array_equal(bits(out[miss]), bits(want[miss]))
    assert np.all(np.isnan(ws[miss])) and not np.array_equal(bits(out[~miss]), bits(want[~miss]))
    # a pixel that is hit skips exactly the taps whose (clamped) neighbour is a miss
    for y, x in zip(*np.nonzero(~miss)):
        for k in range(9):
            yy, xx = min(max(y + k // 3 - 1, 0), 6), min(max(x + k % 3 - 1, 0), 8)
            assert np.isnan(ws[y, x, k]) == bool(miss[yy, xx])


def test_clipped_taps_lie_in_the_box_on_the_segment_to_its_centre():
    rng = np.random.default_rng(7)
    cur = rng.random((6, 6, 4), np.float32)
    n_clipped = 0
    for y in range(6):
        for x in range(6):
            mn, mx = T.box(cur, x, y)
            assert np.all(mn <= mx)
            for _ in range(6):
                q = ((rng.random(3, np.float32) - F(0.5)) * F(200)).astype(np.float32)        # far outside: mapped colours are below 1
                r = T.clip(mn[:3], mx[:3], q)
                c = (0.5 * (mx[:3].astype(np.float64) + mn[:3])).astype(np.float64)
                half = 0.5 * (mx[:3].astype(np.float64) - mn[:3]) + 1e-8
                # inside the box grown by the 1e-8 half-size (and the roundings of values below 1: a few 2^-24)
                assert np.all(np.abs(r - c) <= half + 8 * 2.0 ** -24), (mn, mx, q, r)
                # on the segment q -> centre: r - c = s (q - c) with one s in (0, 1]
                d, e = q.astype(np.float64) - c, r.astype(np.float64) - c
                s = np.dot(d, e) / np.dot(d, d)
                assert 0.0 < s <= 1.0 and np.max(np.abs(e - s * d)) <= 8 * 2.0 ** -24
                n_clipped += s < 1.0
            inside = (c + 0.5 * (rng.random(3) - 0.5) * (mx[:3] - mn[:3])).astype(np.float32)
            assert np.array_equal(bits(T.clip(mn[:3], mx[:3], inside)), bits(inside))
    assert n_clipped == 6 * 6 * 6


def test_weight_zero_keeps_the_mapped_centre_and_the_source_alpha():
    """Nine motions of magnitude 1.5: len2 > 2, so 1 - clamp(len2 / 2) = 0 and no tap counts."""
    rng = np.random.default_rng(8)
    cur = (rng.random((5, 7, 4), np.float32) * F(8)).astype(np.float32)
    hist = (rng.random((5, 7, 4), np.float32) * F(8)).astype(np.float32)
    mot = still(5, 7)
    ang = rng.random((5, 7)) * 6.28
    mot[..., 0] = (1.5 * np.cos(ang)).astype(np.float32)
    mot[..., 1] = (1.5 * np.sin(ang)).astype(np.float32)
    out, _, _, ea, ws = T.resolve(cur, hist, mot, extras=True)
    assert np.all(ws == 0.0)
    for y in range(5):
        for x in range(7):
            assert np.array_equal(bits(out[y, x]), bits(T.sample_color(cur[y, x])))
    assert np.array_equal(out[..., 3], cur[..., 3])


def test_whole_texel_motion_fetches_the_next_texel_exactly():
    """16 x 8 (powers of two, so uv, the rescale of the velocity and the texel coordinate are exact -- checked below): motion (1/w, 0)
    fetches the history texel one to the right with fraction 0, the clamped one at the right edge; (0, -1/h) the one below."""
    w, h = 16, 8
    v = F(1) / F(w)
    len2 = F(F(v * v) + F(1e-6))
    assert F(F(v / len2) * len2) == v
    rng = np.random.default_rng(9)
    hist = (rng.random((h, w, 4), np.float32) * F(8)).astype(np.float32)
    for y in range(h):
        for x in range(w):
            got, uv = T.tap(hist, x, y, [v, 0.0, 1.0, 1.0])
            assert np.array_equal(bits(got), bits(hist[y, min(x + 1, w - 1)])), (x, y)
            got, uv = T.tap(hist, x, y, [0.0, -F(1) / F(h), 1.0, 1.0])
            assert np.array_equal(bits(got), bits(hist[max(y - 1, 0), x])), (x, y)
            # out of the frame on every side, NaN and inf: the edge texel, never a read outside the plane
            for md, (yy, xx) in (([-1.2, 0.0], (y, 0)), ([1.2, 0.0], (y, w - 1)), ([0.0, -1.2], (0, x)), ([0.0, 1.2], (h - 1, x))):
                got, uv = T.tap(hist, x, y, md + [1.0, 1.0])
                assert np.array_equal(bits(got), bits(hist[yy, xx])), (md, x, y)
    for md in ([np.nan, 0.0], [np.inf, -np.inf], [0.0, np.nan], [3e38, 3e38]):
        got, uv = T.tap(hist, 3, 3, md + [1.0, 1.0])
        assert got.shape == (4,)
    # the tap weight of that motion: exp(-2.29 |v|^2) (1 - len2 / 2), a few fp32 roundings
    mot = still(h, w)
    mot[..., 0] = v
    ws = T.resolve(hist, hist, mot, extras=True)[4]
    want = np.exp(-2.29 * float(v) ** 2) * (1.0 - float(len2) / 2.0)
    assert np.max(np.abs(ws.astype(np.float64) - want)) <= 8 * 2.0 ** -24


def test_saturated_input_gives_plus_infinity():
    """(1e8, 1e8, 1e8): 1 + lum rounds to lum, the mapped colour is exactly 1, YCoCg2RGB gives (1, 1, 1), unmap divides by 1 - 1:
    the documented class is +inf in the three colour channels, alpha 1; gamma clamps it to 1 = 255."""
    cur = np.zeros((4, 4, 4), np.float32)
    cur[..., :3] = 1e8
    cur[..., 3] = 0.25
    out, gf, g8 = T.resolve(cur, cur, still(4, 4))
    assert np.all(np.isposinf(out[..., :3])) and np.all(out[..., 3] == 1.0)
    assert np.all(gf == 1.0) and np.all(g8 == 0xffffffff)
    # fed back as history it maps to inf / inf: NaN, stored with the one documented bit pattern; a NaN quantises to 0
    out2, gf2, g82 = T.resolve(cur, out, still(4, 4))
    assert np.all(bits(out2[..., :3]) == 0x7fc00000) and np.all(g82 == 0xff000000)


def test_rgba8_is_round_to_nearest_of_the_clamped_float():
    rng = np.random.default_rng(10)
    halves = ((np.arange(255, dtype=np.float64) + 0.5) / 255.0).astype(np.float32)
    special = np.array([0.0, 1.0, 1.5, 7.0, -0.25, 1e-9, np.nextafter(F(1), F(0)), np.nextafter(F(1), F(2))], np.float32)
    g = np.concatenate([special, halves, np.nextafter(halves, F(0)), np.nextafter(halves, F(2)),
                        rng.random(4096 - 8 - 3 * 255, np.float32) * F(1.25) - F(0.125)]).astype(np.float32)
    assert g.size == 4096
    c = np.minimum(np.maximum(g, F(0)), F(1))
    want = np.floor(c * F(255) + F(0.5)).astype(np.uint32)      # fp32 throughout, as the kernel
    assert np.array_equal(T.unorm8(g), want)
    assert want[0] == 0 and want[1] == 255 and want[2] == 255 and want[4] == 0
    # through the whole pass with gamma 1 (pow(x, 1) = x): R in the low byte, alpha 255
    cur = np.zeros((64, 64, 4), np.float32)
    cur[..., 0] = g.reshape(64, 64); cur[..., 1] = g[::-1].reshape(64, 64); cur[..., 2] = 0.5
    out, gf, g8 = T.resolve(np.maximum(cur, 0), None, still(64, 64), gamma=1.0)
    assert np.array_equal(g8 & 0xff, np.maximum(want.reshape(64, 64), 0))
    assert np.array_equal((g8 >> 8) & 0xff, want[::-1].reshape(64, 64))
    assert np.all((g8 >> 16) & 0xff == 128) and np.all(g8 >> 24 == 255)


@pytest.mark.parametrize("w,h,seed", T.GPU_CASES)
def test_the_gpu_cases_keep_the_exclusion_cap_and_the_still_planes_are_exact(w, h, seed):
    """What tests/test_gpu_taa.py relies on, confirmed without a GPU: on the still planes every exp argument is (-)0, so exp is 1 on any
    libm; on the moving planes the components excluded for 1 - lum < 2^-10 stay below 0.5 % of the finite ones over the three frames."""
    for moving in (False, True):
        frames, hist = T.make_inputs(w, h, seed, moving=moving)
        n_fin = n_exc = 0
        for k, f in enumerate(T.run_twin(frames)):
            assert np.all(np.isnan(f["weights"])) == (k == 0 or (w, h) == (1, 1) and frames[k][1][0, 0, 2] < 0)
            if not moving:
                assert np.all((f["exp_args"] == 0) | np.isnan(f["exp_args"]))
            fin = np.isfinite(f["out"][..., :3])
            n_fin += int(fin.sum())
            n_exc += int((T.excluded(f["out"], f["weights"])[..., None] & fin).sum())
        assert n_exc <= 0.005 * n_fin, (n_exc, n_fin)


def test_lds_pitch_is_conflict_free_for_every_read_the_kernel_makes():
    """The LDS rule (one LDS cycle per lane group; within a group distinct addresses must fall on distinct banks): lane l of a wave reads
    element (l >> 3) * pitch + (l & 7) + constant of the colour (16 B; the compiler reads 12 or 16 of them), motion (8 B) and depth (4 B)
    arrays.  Enumerated for the kernel's pitch; pitch 10 (the bare halo) conflicts."""
    src = open(os.path.join(ROOT, "aten_amd", "csrc", "device", "taa.hpp")).read()
    pitch = int(re.search(r"kTaaPitch = (\d+)", src).group(1))
    assert pitch >= 10

    def ranges(spec):
        return [l for a, b in spec for l in range(a, b + 1)]
    g128 = [ranges(s) for s in ([(0, 3), (12, 15), (20, 27)], [(4, 11), (16, 19), (28, 31)], [(32, 35), (44, 47), (52, 59)], [(36, 43), (48, 51), (60, 63)])]
    g96 = [ranges(s) for s in ([(0, 3), (20, 23)], [(4, 7), (16, 19)], [(8, 11), (28, 31)], [(12, 15), (24, 27)],
                               [(32, 35), (52, 55)], [(36, 39), (48, 51)], [(40, 43), (60, 63)], [(44, 47), (56, 59)])]
    g32 = [list(range(0, 32)), list(range(32, 64))]
    kinds = [("b128", 16, 4, 64, g128), ("b96", 16, 3, 32, g96), ("b64", 8, 2, 64, g32), ("b32", 4, 1, 32, g32)]

    def worst(p, elem, dwords, banks, groups):
        worst_ = 1
        for off in range(0, 3 * p):        # any constant offset (the nine taps, any wave of the block)
            for grp in groups:
                use = {}
                for l in grp:
                    a = ((l >> 3) * p + (l & 7) + off) * elem // 4
                    for d in range(dwords):
                        use.setdefault((a + d) % banks, set()).add(a)
                worst_ = max(worst_, max(len(v) for v in use.values()))
        return worst_
    for name, elem, dwords, banks, groups in kinds:
        assert worst(pitch, elem, dwords, banks, groups) == 1, name
    assert max(worst(10, *k[1:]) for k in kinds) > 1
