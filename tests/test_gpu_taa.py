"""The display tail on the device (aten_amd/csrc/device/taa.hpp; docs/TAA.md) against its CPU twin (tests/cxx/taa_oracle.cpp), its
wiring behind SVGF and ReSTIR frames, scheduling, state and refusals."""
import numpy as np
import pytest

import taa_oracle as T
from aten_amd.renderer import AtenAmdError, PathTracing
from aten_amd.scene.camera import create_camera
from conftest import parity_record

pytestmark = pytest.mark.gpu

INVALID_ARG = -1
DEPTH = 3
# Measured, device against twin, on the moving planes of T.GPU_CASES (all three cases, three frames each; docs/TAA.md has the same
# figures and the parity report gets them on every run).  The assertions below hold 4 x these.
#   MEASURED_REL:   max |device - twin| / (the pixel's largest |colour component| of the twin), finite components, TAA output
#   MEASURED_POW:   max |device gamma float - twin gamma of the DEVICE's TAA output| (values in [0, 1])
#   MEASURED_SHARE: share of RGBA8 colour bytes that differ (by exactly 1) from the twin's
MEASURED_REL = 1.691e-6
MEASURED_POW = 5.96e-8
MEASURED_SHARE = 0.0       # 0 of 24897 bytes: with 4 x 0 the planes must agree byte for byte


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def status_of(call):
    with pytest.raises(AtenAmdError) as e:
        call()
    return int(str(e.value).rsplit("(status ", 1)[1].rstrip(")"))


def device_frames(r, frames, hist=None, gamma=T.GAMMA):
    """The frames through atn_taa_resolve, source 2; the same dicts as T.run_twin (without the extras) + previous_history."""
    res = []
    if hist is not None:
        r.taa_upload("history", hist)
    for col, mot in frames:
        h, w = col.shape[:2]
        r.taa_upload("color", col)
        r.taa_upload("motion_depth", mot)
        gf, g8 = r.taa_resolve(w, h, "uploaded", gamma=gamma, want_float=True, want_rgba8=True)
        res.append(dict(out=r.taa_buffer("output"), gamma=gf, rgba8=g8, rgba8_again=r.taa_buffer("rgba8"), gamma_again=r.taa_buffer("gamma"),
                        previous_history=r.taa_buffer("previous_history")))
    return res


def as_bytes(g8_u32):
    return np.ascontiguousarray(g8_u32, np.uint32).view(np.uint8).reshape(g8_u32.shape + (4,))


@pytest.fixture(scope="module")
def ctx():
    r = PathTracing(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def twin():
    """The twin's frames of every case, still and moving, computed once."""
    out = {}
    for w, h, seed in T.GPU_CASES:
        for moving in (False, True):
            frames, hist = T.make_inputs(w, h, seed, moving=moving)
            out[(w, h, moving)] = (frames, hist, T.run_twin(frames))
    return out


# ---- 1. the exact part ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,seed", T.GPU_CASES)
def test_still_planes_equal_the_twin_byte_for_byte(ctx, twin, w, h, seed):
    """All motion zero: every exp argument is -0 (checked on the twin's exported arguments), exp is 1 on both sides, and every other
    operation of the pass is one IEEE rounding: output, history and RGBA8-of-own-float are byte-equal for three frames, NaN and inf
    included.  The first frame has no history and passes through."""
    frames, hist, want = twin[(w, h, False)]
    ctx.taa_reset()
    got = device_frames(ctx, frames)
    for k, (g, t) in enumerate(zip(got, want)):
        assert np.all((t["exp_args"] == 0) | np.isnan(t["exp_args"]))
        assert np.array_equal(bits(g["out"]), bits(t["out"])), k
        if k == 0:
            first = frames[0][0].copy(); first[..., 3] = 1.0
            assert np.array_equal(bits(g["out"]), bits(first))
        else:
            assert np.array_equal(bits(g["previous_history"]), bits(got[k - 1]["out"])), k
        assert np.array_equal(g["rgba8"], as_bytes(T.unorm8(g["gamma"][..., :3]).reshape(h, w, 3) @ np.array([1, 256, 65536], np.uint32) | 0xff000000)), k
        assert np.array_equal(g["rgba8"], g["rgba8_again"]) and np.array_equal(bits(g["gamma"]), bits(g["gamma_again"]))
    if min(w, h) >= 8:
        assert np.isinf(got[1]["out"]).any() and np.isnan(got[2]["out"]).any()


def test_uploaded_history_is_the_first_frames_history(ctx, twin):
    w, h, seed = T.GPU_CASES[1]
    frames, hist, _ = twin[(w, h, False)]
    want = T.run_twin(frames[:1], hist)
    ctx.taa_reset()
    got = device_frames(ctx, frames[:1], hist)
    assert np.array_equal(bits(got[0]["out"]), bits(want[0]["out"]))
    assert np.array_equal(bits(got[0]["previous_history"]), bits(hist))
    assert not np.all(np.isnan(want[0]["weights"]))


# ---- 2. moving planes ------------------------------------------------------------------------------------------------------------------
def test_moving_planes_agree_within_the_measured_libm_bounds(ctx, twin):
    """expf (ocml against glibc) differs in the last bit, and unmap's 1 / (1 - lum) amplifies it: finite components agree within
    4 x the measured maximum (relative to the pixel's largest colour component), non-finite ones in class and sign; components of pixels
    that unmap divided by less than 2^-10 are left out (at most 0.5 %: tests/test_taa_oracle_cpu.py confirms the twin's count).  The
    gamma plane is held to powf's measured bound on the device's own TAA output, RGBA8 to the quantisation of the device's own float
    plane exactly and to the twin's within 1 in at most 4 x the measured share of bytes."""
    worst_rel = worst_pow = 0.0
    n_bytes = n_diff = n_fin = n_exc = 0
    for w, h, seed in T.GPU_CASES:
        frames, hist, want = twin[(w, h, True)]
        ctx.taa_reset()
        got = device_frames(ctx, frames)
        for k, (g, t) in enumerate(zip(got, want)):
            go, to = g["out"], t["out"]
            with np.errstate(all="ignore"):
                assert np.array_equal(np.isnan(go), np.isnan(to)), (w, h, k)
                assert np.array_equal(np.isinf(go), np.isinf(to)) and np.array_equal(np.signbit(go)[np.isinf(to)], np.signbit(to)[np.isinf(to)]), (w, h, k)
                assert np.array_equal(go[..., 3], to[..., 3])
                fin = np.isfinite(to[..., :3])
                exc = T.excluded(to, t["weights"])[..., None] & fin
                scale = np.max(np.where(fin, np.abs(to[..., :3]), 0.0), axis=-1, keepdims=True)
                rel = np.where(fin & ~exc & (scale > 0), np.abs(go[..., :3].astype(np.float64) - to[..., :3]) / np.maximum(scale, 1e-30), 0.0)
            n_fin += int(fin.sum()); n_exc += int(exc.sum())
            if min(w, h) >= 8 and k:
                assert (np.isinf(to) if k == 1 else np.isnan(to)).any()
            worst_rel = max(worst_rel, float(rel.max()))
            # gamma: the device's float plane against the twin's pow of the DEVICE's TAA output (enable = 0 passes it through)
            own = T.resolve(go, None, frames[k][1], enable=False, gamma=T.GAMMA)
            with np.errstate(all="ignore"):
                assert np.array_equal(np.isnan(g["gamma"]), np.isnan(own[1]))
                worst_pow = max(worst_pow, float(np.nanmax(np.abs(g["gamma"].astype(np.float64) - own[1]), initial=0.0)))
            assert np.array_equal(g["rgba8"][..., :3], T.unorm8(g["gamma"][..., :3]).reshape(h, w, 3).astype(np.uint8)) and np.all(g["rgba8"][..., 3] == 255)
            d8 = np.abs(g["rgba8"][..., :3].astype(np.int32) - as_bytes(t["rgba8"])[..., :3].astype(np.int32))
            ok = ~(exc.any(-1) | ~fin.all(-1))[..., None] & np.ones(3, bool)
            assert d8[ok].max(initial=0) <= 1, (w, h, k)
            n_bytes += int(ok.sum()); n_diff += int((d8[ok] != 0).sum())
    share = n_diff / max(n_bytes, 1)
    parity_record("taa_moving_planes", np.zeros(1, np.float32), np.zeros(1, np.float32), taa_max_rel=worst_rel, taa_max_pow_abs=worst_pow,
                  taa_rgba8_share_off_by_one=share, taa_finite_components=n_fin, taa_excluded_components=n_exc,
                  bounds=dict(rel=4 * MEASURED_REL, pow=4 * MEASURED_POW, share=4 * MEASURED_SHARE))
    print("taa moving planes: max rel %.4g  max pow abs %.4g  rgba8 share %.4g (%d of %d)  excluded %d of %d"
          % (worst_rel, worst_pow, share, n_diff, n_bytes, n_exc, n_fin))
    assert n_exc <= 0.005 * n_fin
    assert worst_rel <= 4 * MEASURED_REL
    assert worst_pow <= 4 * MEASURED_POW
    assert share <= 4 * MEASURED_SHARE


# ---- 3. wiring -------------------------------------------------------------------------------------------------------------------------
def scene_context(fs, cam, w, h, fif=1, geometry_motion=False):
    r = PathTracing(0)
    try:
        r.UpdateSceneData(fs)
        r.updateCamera(create_camera(cam["pos"], cam["at"], cam["vfov"], w, h))
        r.initSampler(w, h, 0)
        r.set_frames_in_flight(fif)
        if geometry_motion:
            r.set_geometry_motion(True)
    except Exception:
        r.close()
        raise
    return r


@pytest.fixture(scope="module")
def cornell():
    from aten_amd.scene import scenedefs
    return scenedefs.cornell_box()


def moved(cam, k):
    return dict(cam, pos=(cam["pos"][0] + 0.05 * k, cam["pos"][1], cam["pos"][2]))


def resolve_uploaded(b, color, motion, history, w, h):
    """The same frame through source 2 of another context with the given history (None: none)."""
    b.taa_reset()
    if history is not None:
        b.taa_upload("history", history)
    b.taa_upload("color", color)
    b.taa_upload("motion_depth", motion)
    g8 = b.taa_resolve(w, h, "uploaded", want_rgba8=True)
    return b.taa_buffer("output"), g8


@pytest.mark.parametrize("renderer", ["svgf", "restir"])
def test_resolving_behind_a_frame_equals_resolving_its_downloaded_planes(ctx, cornell, renderer):
    fs, cam = cornell
    w = h = 64
    r = scene_context(fs, cam, w, h)
    try:
        history = None
        for k in range(2):
            r.updateCamera(create_camera(moved(cam, k)["pos"], cam["at"], cam["vfov"], w, h))
            if renderer == "svgf":
                r.svgf_render(w, h, DEPTH, 3, frame=k, compute_motion=1, download=False)
                g8 = r.taa_resolve(w, h, "svgf", want_rgba8=True)
                color, motion = r.svgf_buffer("output"), r.svgf_buffer("motion_depth")
            else:
                r.restir_render(w, h, DEPTH, 3, frame=k, compute_motion=1, download=False)
                g8 = r.taa_resolve(w, h, "restir", want_rgba8=True)
                color, motion = r.download_film(), r.restir_buffer("motion")
            out = r.taa_buffer("output")
            want, want8 = resolve_uploaded(ctx, color, motion, history, w, h)
            assert np.array_equal(bits(out), bits(want)) and np.array_equal(g8, want8), k
            if k:
                assert np.count_nonzero(motion[..., :2]) > 0 and not np.array_equal(bits(out[..., :3]), bits(color[..., :3]))
            history = out
    finally:
        r.close()


def test_resolving_behind_a_geometry_motion_frame_of_the_skinned_room(ctx):
    from test_gpu_motion import Skinned
    sk = Skinned(n_ticks=2)
    w, h = 100, 52
    r = scene_context(sk.fs0, sk.cam, w, h, geometry_motion=True)
    try:
        skin = sk.create_skin(r)
        sk.tick(r, skin, 0)
        r.svgf_render(w, h, DEPTH, 3, frame=0, compute_motion=2, download=False)
        r.taa_resolve(w, h, "svgf")
        history = r.taa_buffer("output")
        sk.tick(r, skin, 1)
        r.svgf_render(w, h, DEPTH, 3, frame=1, compute_motion=2, download=False)
        g8 = r.taa_resolve(w, h, "svgf", want_rgba8=True)
        color, motion = r.svgf_buffer("output"), r.svgf_buffer("motion_depth")
        assert np.count_nonzero(motion[..., :2]) > 0
        want, want8 = resolve_uploaded(ctx, color, motion, history, w, h)
        assert np.array_equal(bits(r.taa_buffer("output")), bits(want)) and np.array_equal(g8, want8)
    finally:
        r.close()


# ---- 4. scheduling and state -------------------------------------------------------------------------------------------------------------
def test_three_frames_in_flight_equal_one(cornell):
    """Four SVGF frames, each with its display tail behind it: the first two enqueued without any host wait, the last two waiting for
    their RGBA8 only."""
    fs, cam = cornell
    w = h = 64
    outs = {}
    for fif in (1, 3):
        r = scene_context(fs, cam, w, h, fif=fif)
        try:
            got = []
            for k in range(4):
                r.svgf_render(w, h, DEPTH, 3, frame=k, compute_motion=1, download=False)
                g8 = r.taa_resolve(w, h, "svgf", want_rgba8=k >= 2)
                if k >= 2:
                    got.append(g8.copy())
            got += [r.taa_buffer(n) for n in ("output", "previous_history", "rgba8")] + [r.svgf_buffer("output")]
            outs[fif] = got
        finally:
            r.close()
    for i, (x, y) in enumerate(zip(outs[1], outs[3])):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), i


def test_reset_and_a_size_change_bring_back_the_first_frame_rule(ctx, twin):
    w, h, seed = T.GPU_CASES[1]
    frames, hist, want = twin[(w, h, True)]
    ctx.taa_reset()
    got = device_frames(ctx, frames[:2])
    assert not np.array_equal(bits(got[1]["out"][..., :3]), bits(frames[1][0][..., :3]))        # frame 1 used its history
    ctx.taa_reset()
    again = device_frames(ctx, frames[1:2])
    through = frames[1][0].copy(); through[..., 3] = 1.0
    assert np.array_equal(bits(again[0]["out"]), bits(through))
    # enable = 0 passes through and still advances the history
    ctx.taa_upload("color", frames[2][0]); ctx.taa_upload("motion_depth", frames[2][1])
    ctx.taa_resolve(w, h, "uploaded", enable=False)
    off = frames[2][0].copy(); off[..., 3] = 1.0
    assert np.array_equal(bits(ctx.taa_buffer("output")), bits(off)) and np.array_equal(bits(ctx.taa_buffer("previous_history")), bits(through))
    # another size: no history at that size, whatever happened before; and back again: none either
    w2, h2, seed2 = T.GPU_CASES[2]
    f2 = twin[(w2, h2, True)][0]
    other = device_frames(ctx, f2[:1])
    t2 = f2[0][0].copy(); t2[..., 3] = 1.0
    assert np.array_equal(bits(other[0]["out"]), bits(t2))
    back = device_frames(ctx, frames[:1])
    t0 = frames[0][0].copy(); t0[..., 3] = 1.0
    assert np.array_equal(bits(back[0]["out"]), bits(t0))


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals(cornell):
    fs, cam = cornell
    w = h = 32
    r = scene_context(fs, cam, w, h)
    try:
        plane = np.zeros((h, w, 4), np.float32)
        r._taa_size = (h, w)
        assert status_of(lambda: r.taa_buffer("output")) == INVALID_ARG                 # nothing resolved yet
        assert status_of(lambda: r.taa_resolve(w, h, "svgf")) == INVALID_ARG            # no SVGF frame
        assert status_of(lambda: r.taa_resolve(w, h, "restir")) == INVALID_ARG          # no ReSTIR frame
        assert status_of(lambda: r.taa_resolve(w, h, "uploaded")) == INVALID_ARG        # no planes
        r.taa_upload("color", plane)
        assert status_of(lambda: r.taa_resolve(w, h, "uploaded")) == INVALID_ARG        # no motion/depth plane
        r.taa_upload("motion_depth", plane)
        assert status_of(lambda: r.taa_resolve(w + 1, h, "uploaded")) == INVALID_ARG    # another size than the planes'
        for gamma in (0.0, -2.2, float("nan"), float("inf")):
            assert status_of(lambda: r.taa_resolve(w, h, "uploaded", gamma=gamma)) == INVALID_ARG
        assert status_of(lambda: r._check(r._l.atn_taa_resolve(r._ctx, 3, w, h, 1, 2.2, None, None))) == INVALID_ARG
        assert status_of(lambda: r._check(r._l.atn_taa_resolve(r._ctx, 2, 0, h, 1, 2.2, None, None))) == INVALID_ARG
        assert status_of(lambda: r._check(r._l.atn_taa_upload(r._ctx, 5, w, h, plane.ctypes.data))) == INVALID_ARG
        assert status_of(lambda: r._check(r._l.atn_taa_upload(r._ctx, 0, w, h, None))) == INVALID_ARG
        r.taa_resolve(w, h, "uploaded")
        assert status_of(lambda: r.taa_buffer("gamma")) == INVALID_ARG                  # the float plane was not asked for
        assert status_of(lambda: r._check(r._l.atn_taa_download(r._ctx, 7, plane.ctypes.data))) == INVALID_ARG
        assert r._l.atn_taa_output_device(r._ctx)
        # a frame of each renderer: its own size only
        r.svgf_render(w, h, DEPTH, 3, frame=0, compute_motion=1, download=False)
        r.taa_resolve(w, h, "svgf")
        assert status_of(lambda: r.taa_resolve(w, h + 1, "svgf")) == INVALID_ARG
        assert status_of(lambda: r.taa_resolve(w, h, "restir")) == INVALID_ARG
        r.restir_render(w, h, DEPTH, 3, frame=0, compute_motion=1, download=False)
        r.taa_resolve(w, h, "restir")
        assert status_of(lambda: r.taa_resolve(w + 8, h, "restir")) == INVALID_ARG
        # the renderers' resets take their frames away, not the history
        r.svgf_reset(); r.restir_reset()
        assert status_of(lambda: r.taa_resolve(w, h, "svgf")) == INVALID_ARG
        assert status_of(lambda: r.taa_resolve(w, h, "restir")) == INVALID_ARG
        # ... and a frame without a motion/depth plane is refused by the renderer itself, so the tail never sees one
        assert status_of(lambda: r.svgf_render(w, h, DEPTH, 3, frame=0, compute_motion=0, download=False)) == INVALID_ARG
        assert status_of(lambda: r.taa_resolve(w, h, "svgf")) == INVALID_ARG
    finally:
        r.close()
