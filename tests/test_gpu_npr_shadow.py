"""The NPR shadow pre-pass on the GPU (atn_npr_shadow_*, device/npr_shadow.hpp) against the CPU restatement of the reference
(tests/cxx/npr_shadow_oracle.cpp): the row filter as a stage, the pre-pass's planes, the frames that read the plane, a camera move
without a re-upload, the byte-equality rules and the refused configurations.  docs/NPR_SHADOW.md has the decisions and the numbers."""
import numpy as np
import pytest

from conftest import make_camera, parity_record
from test_gpu_parity import frame_tolerance_report

pytestmark = pytest.mark.gpu

SIZES = [(112, 112), (100, 52)]
FRAMES = (0, 3)
ERR_INVALID_ARG, ERR_UNSUPPORTED = -1, -5     # include/aten_amd.h
# The filter's bound, derived: the device's expf and the host's differ by at most ~2 ulp per weight, eleven-term sums and one division
# add ~24 roundings: at most ~32 * 2^-24 ~ 2e-6 on a value in [0, 1], doubled.
FILTER_TOL = 4e-6
CAM2 = dict(pos=(0.45, 1.25, 3.0), at=(0.0, 0.9, 0.0), vfov=56.0)


@pytest.fixture(scope="module")
def sq():
    import npr_shadow_oracle
    npr_shadow_oracle.lib()
    return npr_shadow_oracle


@pytest.fixture(scope="module")
def twin(orc, sq):
    """The twin's pre-pass, computed once per (pane, camera, size, frame) and shared: dict lit, depth, plane, mtrl, toon + the scene
    (never plugged: the GPU's), the camera and the seeds."""
    from aten_amd import layout as L
    from aten_amd.scene import scenedefs
    cache, scenes = {}, {}

    def get(pane, w, h, frame, cam=None):
        key = (pane, w, h, frame, cam is not None)
        if key not in cache:
            if pane not in scenes:
                scenes[pane] = scenedefs.stylized_shadow_room(alpha_blocker=pane)
            fs, cam0 = scenes[pane]
            c = make_camera(orc, cam or cam0, w, h)
            seeds = orc.init_sampler(w, h, 0)
            r = sq.prepass(fs, c, seeds, w, h, frame=frame)
            r["toon"] = (r["mtrl"] >= 0) & np.isin(fs.arrays["materials"]["type"][r["mtrl"].clip(0)], (L.MTRL_TOON, L.MTRL_STYLIZED))
            r.update(fs=fs, c=c, seeds=seeds)
            cache[key] = r
        return cache[key]
    return get


def _ctx(fs, c, w, h, mode=1):
    from aten_amd.renderer import PathTracing
    r = PathTracing(0)
    r.UpdateSceneData(fs)
    r.updateCamera(c)
    r.initSampler(w, h, 0)
    r.set_npr_shadow(mode)
    return r


def _plugged(sq, pane, plane):
    """A scene of its own for the CPU frame reference, the plane in its screen_space_texture."""
    from aten_amd.scene import scenedefs
    fs, _ = scenedefs.stylized_shadow_room(alpha_blocker=pane)
    return sq.plug_plane(fs, plane)


def _window_agrees(agree):
    """Pixels all of whose 11 taps (x clamped to the row) agree."""
    h, w = agree.shape
    out = np.ones_like(agree)
    xs = np.arange(w)
    for i in range(-5, 6):
        out &= agree[:, np.clip(xs + i, 0, w - 1)]
    return out


# ---- 1. the filter as a stage
def test_filter_stage(gpu, sq, twin):
    inf = np.float32(np.inf)
    rng = np.random.default_rng(11)
    cases = [("room %dx%d" % (w, h), twin(False, w, h, 0)["lit"], twin(False, w, h, 0)["depth"]) for w, h in SIZES]
    for w, h in ((13, 3), (7, 2), (1, 1)):
        lit = (rng.uniform(size=(h, w)) < 0.5).astype(np.float32)
        depth = rng.uniform(1.0, 1.5, (h, w)).astype(np.float32)
        depth[rng.uniform(size=(h, w)) < 0.25] = inf
        if (w, h) == (1, 1):
            depth[0, 0] = inf
        lit[np.isinf(depth)] = 0.0
        cases.append(("synthetic %dx%d" % (w, h), lit, depth))
    cases.append(("synthetic 1x1 hit", np.float32([[1.0]]), np.float32([[2.5]])))
    worst = 0.0
    for name, lit, depth in cases:
        got, want = gpu.npr_shadow_filter(lit, depth), sq.row_filter(lit, depth)
        miss = np.isinf(depth)
        assert np.all(got[miss] == 1.0) and np.all(want[miss] == 1.0), name
        err = float(np.abs(got[~miss].astype(np.float64) - want[~miss]).max()) if (~miss).any() else 0.0
        print("filter stage, %s: max |gpu - twin| = %.3g on %d pixels (%d miss-centred, exactly 1)" % (name, err, (~miss).sum(), miss.sum()))
        parity_record("NPR shadow filter stage, %s" % name, got[..., None].repeat(3, -1), want[..., None].repeat(3, -1), tol=FILTER_TOL,
                      max_abs_err_hit_centred=err)
        worst = max(worst, err)
        assert err <= FILTER_TOL, (name, err)
    print("filter stage: worst %.3g (bound %g)" % (worst, FILTER_TOL))
    # sizes outside 1..16384 and null planes are invalid arguments
    one = np.zeros((1, 1), np.float32)
    assert gpu._l.atn_npr_shadow_filter(gpu._ctx, one.ctypes.data, one.ctypes.data, 0, 1, one.ctypes.data) == ERR_INVALID_ARG
    assert gpu._l.atn_npr_shadow_filter(gpu._ctx, one.ctypes.data, one.ctypes.data, 1, 16385, one.ctypes.data) == ERR_INVALID_ARG
    assert gpu._l.atn_npr_shadow_filter(gpu._ctx, None, one.ctypes.data, 1, 1, one.ctypes.data) == ERR_INVALID_ARG


# ---- 2. the pre-pass's planes
@pytest.mark.parametrize("pane", [False, True])
@pytest.mark.parametrize("w,h", SIZES)
def test_prepass_stage(gpu, twin, pane, w, h):
    t0 = twin(pane, w, h, 0)
    r = _ctx(t0["fs"], t0["c"], w, h)
    try:
        for f in FRAMES:
            t = twin(pane, w, h, f)
            r.reset()
            r.render(w, h, frame=f, download=False)
            depth, lit, plane = r.npr_shadow_buffer("depth"), r.npr_shadow_buffer("lit"), r.npr_shadow_buffer("plane")
            assert np.array_equal(depth.view(np.uint32), t["depth"].view(np.uint32))         # bit-equal, misses +inf
            assert set(np.unique(lit)) <= {0.0, 1.0}
            agree = lit == t["lit"]
            win = _window_agrees(agree)
            err = float(np.abs(plane[win].astype(np.float64) - t["plane"][win]).max())
            print("pre-pass stage, pane %d %dx%d frame %d: lit equal %.4f %%, windows that agree %.4f %%, plane max err there %.3g"
                  % (pane, w, h, f, 100 * agree.mean(), 100 * win.mean(), err))
            parity_record("NPR shadow pre-pass, pane %d %dx%d frame %d" % (pane, w, h, f), plane[..., None].repeat(3, -1),
                          t["plane"][..., None].repeat(3, -1), tol=FILTER_TOL, lit_equal=float(agree.mean()), windows_agree=float(win.mean()),
                          plane_max_err_where_windows_agree=err)
            assert agree.mean() >= 0.995, agree.mean()
            assert win.mean() >= 0.94, win.mean()
            assert err <= FILTER_TOL, err
            miss = np.isinf(depth)
            assert miss.any() and np.all(plane[miss] == 1.0) and not lit[miss].any()
    finally:
        r.close()


def test_prepass_without_the_base_material_flag(gpu, orc, sq):
    """enable_shadowray_base_stylized_shadow = 0: a first-hit toon surface draws its target-light sample and casts no ray; the
    walls' rays (and the dimensions they are drawn from) are unchanged."""
    from aten_amd import layout as L
    from aten_amd.scene import scenedefs
    w, h = 100, 52
    fs, cam = scenedefs.stylized_shadow_room()
    fs.desc.enable_shadowray_base_stylized_shadow = 0
    c = make_camera(orc, cam, w, h)
    t = sq.prepass(fs, c, orc.init_sampler(w, h, 0), w, h, frame=3)
    toon = (t["mtrl"] >= 0) & np.isin(fs.arrays["materials"]["type"][t["mtrl"].clip(0)], (L.MTRL_TOON, L.MTRL_STYLIZED))
    r = _ctx(fs, c, w, h)
    try:
        r.render(w, h, frame=3, download=False)
        lit, plane = r.npr_shadow_buffer("lit"), r.npr_shadow_buffer("plane")
    finally:
        r.close()
    assert toon.sum() > 500 and not lit[toon].any() and lit[~toon].sum() > 500
    agree = lit == t["lit"]
    assert agree.mean() >= 0.995
    win = _window_agrees(agree)
    assert win.mean() >= 0.94 and np.abs(plane[win].astype(np.float64) - t["plane"][win]).max() <= FILTER_TOL


# ---- 3. the frames that read the plane
@pytest.mark.parametrize("spp", [1, 4])
def test_render_frames(gpu, orc, sq, twin, spp):
    w, h = 112, 112
    t0 = twin(False, w, h, 0)
    r = _ctx(t0["fs"], t0["c"], w, h)
    try:
        for f in FRAMES:
            t = twin(False, w, h, f)
            r.reset()
            got = r.render(w, h, 5, 3, spp=spp, frame=f)
            want = orc.render(_plugged(sq, False, t["plane"]), t["c"], t["seeds"], w, h, 5, 3, spp=spp, frame=f)
            frac, mean_err = frame_tolerance_report(got, want)
            m = parity_record("NPR shadow frame, atn_render mode 1 112x112 spp %d frame %d" % (spp, f), got, want)
            print("atn_render mode 1, spp %d frame %d: within tolerance %.4f %%, mean err %.3g" % (spp, f, 100 * frac, mean_err), m["max_abs_err"])
            assert frac >= 0.995 and mean_err <= 5e-3, (frac, mean_err)
    finally:
        r.close()


def test_npr_render_frames(gpu, orc, sq, twin):
    """atn_npr_render (lines on) in mode 1 against the NPR twin with the plane plugged in."""
    import npr_oracle
    from aten_amd.scene import scenedefs
    w, h = 112, 112
    fs_gpu, _ = scenedefs.with_feature_lines(scenedefs.stylized_shadow_room())
    t0 = twin(False, w, h, 0)
    r = _ctx(fs_gpu, t0["c"], w, h)
    o = npr_oracle.NPR()
    try:
        for f in FRAMES:
            t = twin(False, w, h, f)
            fs_ref, _ = scenedefs.with_feature_lines((_plugged(sq, False, t["plane"]), None))
            r.npr_reset(); o.reset()
            got = r.npr_render(w, h, frame=f)
            want = o.render(fs_ref, t["c"], t["seeds"], w, h, frame=f)
            frac, mean_err = frame_tolerance_report(got, want)
            parity_record("NPR shadow frame, atn_npr_render mode 1 112x112 frame %d" % f, got, want)
            print("atn_npr_render mode 1, frame %d: within tolerance %.4f %%, mean err %.3g" % (f, 100 * frac, mean_err))
            assert frac >= 0.995 and mean_err <= 5e-3, (frac, mean_err)
            plane = r.npr_shadow_buffer("plane")
            win = _window_agrees(r.npr_shadow_buffer("lit") == t["lit"])
            assert np.abs(plane[win] - t["plane"][win]).max() <= FILTER_TOL       # the same pre-pass as with lines off
    finally:
        r.close(); o.close()


def test_mode_1_darkens_the_toon_pixels_as_the_twin_says(gpu, orc, sq, twin):
    """THE test that fails without the feature: on toon pixels the mode-1 film is darker in sum than the mode-0 film by the factor
    the twin's two films show (the plane plugged in / no texture), +- 2 %."""
    w, h, f = 112, 112, 3
    t = twin(False, w, h, f)
    r = _ctx(t["fs"], t["c"], w, h, mode=0)
    try:
        film0 = r.render(w, h, 5, 3, frame=f)
        r.set_npr_shadow(1)
        r.reset()
        film1 = r.render(w, h, 5, 3, frame=f)
    finally:
        r.close()
    want1 = orc.render(_plugged(sq, False, t["plane"]), t["c"], t["seeds"], w, h, 5, 3, frame=f)
    want0 = orc.render(t["fs"], t["c"], t["seeds"], w, h, 5, 3, frame=f)
    toon = t["toon"]
    ratio_twin = float(want1[toon][:, :3].sum() / want0[toon][:, :3].sum())
    ratio_gpu = float(film1[toon][:, :3].sum() / film0[toon][:, :3].sum())
    print("toon pixels %d: mode 1 / mode 0 in sum: gpu %.5f, twin %.5f" % (toon.sum(), ratio_gpu, ratio_twin))
    assert ratio_twin < 0.97                                    # the scene does show the term
    assert abs(ratio_gpu - ratio_twin) <= 0.02 * ratio_twin, (ratio_gpu, ratio_twin)
    assert not np.array_equal(film0, film1)
    assert np.array_equal(film0[~toon], film1[~toon])           # nothing but toon shading reads the plane (one sample, depth-0 toon paths end)


# ---- 4. it follows the camera
def test_follows_the_camera(gpu, orc, sq, twin):
    w, h, f = 112, 112, 0
    a, b = twin(False, w, h, f), twin(False, w, h, f, cam=CAM2)
    r = _ctx(a["fs"], a["c"], w, h)
    try:
        first = r.render(w, h, 5, 3, frame=f)
        plane_a = r.npr_shadow_buffer("plane")
        r.updateCamera(b["c"])          # no re-upload
        r.reset()
        got = r.render(w, h, 5, 3, frame=f)
        plane_b, lit_b, depth_b = r.npr_shadow_buffer("plane"), r.npr_shadow_buffer("lit"), r.npr_shadow_buffer("depth")
    finally:
        r.close()
    assert np.array_equal(depth_b.view(np.uint32), b["depth"].view(np.uint32))
    agree = lit_b == b["lit"]
    win = _window_agrees(agree)
    assert agree.mean() >= 0.995 and win.mean() >= 0.94
    assert np.abs(plane_b[win].astype(np.float64) - b["plane"][win]).max() <= FILTER_TOL
    want = orc.render(_plugged(sq, False, b["plane"]), b["c"], b["seeds"], w, h, 5, 3, frame=f)
    frac, mean_err = frame_tolerance_report(got, want)
    print("second camera: lit equal %.4f %%, frame within tolerance %.4f %%, mean err %.3g" % (100 * agree.mean(), 100 * frac, mean_err))
    assert frac >= 0.995 and mean_err <= 5e-3, (frac, mean_err)
    assert (np.abs(plane_a - plane_b) > 0.5).sum() > 200 and not np.array_equal(first, got)
    win_a = _window_agrees(np.abs(plane_a - a["plane"]) <= FILTER_TOL)      # (plane_a is the first camera's)
    assert win_a.mean() >= 0.94


# ---- 5. byte-equality
def _films(fs, c, w, h, mode, in_flight, frames=6, spp=1):
    r = _ctx(fs, c, w, h, mode=mode)
    try:
        r.set_frames_in_flight(in_flight)
        for f in range(frames):
            r.render(w, h, 5, 3, spp=spp, frame=f, download=False)
        film = r.download_film()
        plane = r.npr_shadow_buffer("plane") if mode == 1 else None
    finally:
        r.close()
    return film, plane


def test_byte_equality(gpu, orc, twin):
    from aten_amd.scene import scenedefs
    w, h = 100, 52
    t = twin(False, w, h, 0)
    one, plane1 = _films(t["fs"], t["c"], w, h, 1, 1)
    four, plane4 = _films(t["fs"], t["c"], w, h, 1, 4)
    again, _ = _films(t["fs"], t["c"], w, h, 1, 4)
    assert np.array_equal(one, four) and np.array_equal(plane1, plane4)     # frames in flight: the event orders the plane's readers
    assert np.array_equal(four, again)                                      # two runs
    multi1, _ = _films(t["fs"], t["c"], w, h, 1, 1, frames=3, spp=4)
    multi4, _ = _films(t["fs"], t["c"], w, h, 1, 4, frames=3, spp=4)
    assert np.array_equal(multi1, multi4)
    # mode 0 after mode-1 frames is a fresh context's mode 0: the uploaded texture (none here) is back, no state is left behind
    fresh, _ = _films(t["fs"], t["c"], w, h, 0, 1)
    r = _ctx(t["fs"], t["c"], w, h, mode=1)
    try:
        for f in range(3):
            r.render(w, h, 5, 3, frame=f, download=False)
        r.set_npr_shadow(0)
        r.reset()
        for f in range(6):
            r.render(w, h, 5, 3, frame=f, download=False)
        assert np.array_equal(r.download_film(), fresh)
    finally:
        r.close()
    assert not np.array_equal(fresh, one)
    # a scene whose materials do not enable the term skips the pre-pass: mode 1 is mode 0, and no plane exists
    fs, cam = scenedefs.toon_room()
    c = make_camera(orc, cam, w, h)
    m0, _ = _films(fs, c, w, h, 0, 1, frames=2)
    r = _ctx(fs, c, w, h, mode=1)
    try:
        for f in range(2):
            r.render(w, h, 5, 3, frame=f, download=False)
        assert np.array_equal(r.download_film(), m0)
        out = np.zeros((h, w), np.float32)
        assert r._l.atn_npr_shadow_download(r._ctx, 0, out.ctypes.data, out.size) == ERR_INVALID_ARG
    finally:
        r.close()


# ---- 6. refusals
def test_refused(gpu, orc, twin):
    """Every refusal returns ATN_ERR_UNSUPPORTED (a bad mode or download ATN_ERR_INVALID_ARG) with a message, and the context renders
    a correct mode-0 frame afterwards."""
    import ctypes as C
    from aten_amd import layout as L
    from aten_amd.renderer import Destination
    from aten_amd.scene import scenedefs
    w, h = 100, 52
    t = twin(False, w, h, 0)
    fs, c = t["fs"], t["c"]
    r0 = _ctx(fs, c, w, h, mode=0)
    try:
        mode0 = r0.render(w, h, 5, 3, frame=0)
    finally:
        r0.close()

    def refused(scene, setup, undo, call=None, expect=mode0, **kw):
        r = _ctx(scene, c, w, h, mode=1)
        try:
            setup(r)
            with pytest.raises(Exception) as e:
                (call or (lambda q: q.render(w, h, 5, 3, frame=0, **kw)))(r)
            assert "(status %d)" % ERR_UNSUPPORTED in str(e.value), str(e.value)
            assert len(str(e.value)) > len("(status -5)") + 10, str(e.value)
            undo(r)
            r.set_npr_shadow(0)
            r.reset()
            film = r.render(w, h, 5, 3, frame=0)
            if expect is not None:
                assert np.array_equal(film, expect)
        finally:
            r.close()

    nothing = lambda r: None
    refused(fs, lambda r: r.setScreenShard(0, 2), lambda r: r.setScreenShard(0, 1))
    refused(fs, lambda r: r.set_regeneration(True), lambda r: r.set_regeneration(False))
    refused(fs, nothing, nothing, call=lambda r: r.render_burst(w, h, 2, 5, 3, frame=0))
    refused(fs, lambda r: r.set_shade_math(True), lambda r: r.set_shade_math(False))
    refused(fs, nothing, nothing, count_stats=True)
    car = scenedefs.cornell_box_variant(extra_materials="carpaint")
    assert (car[0].arrays["materials"]["type"] == L.MTRL_CARPAINT).any()
    refused(car[0], nothing, nothing, expect=None)
    # atn_npr_render refuses the same while the mode is on
    lines, _ = scenedefs.with_feature_lines(scenedefs.stylized_shadow_room())
    refused(lines, lambda r: r.set_shade_math(True), lambda r: r.set_shade_math(False), call=lambda r: r.npr_render(w, h, frame=0), expect=None)
    # the mode's values, and a download before any frame has run the pre-pass / with another size
    r = _ctx(fs, c, w, h, mode=0)
    try:
        for bad in (-1, 2, 7):
            assert r._l.atn_npr_shadow_set_mode(r._ctx, bad) == ERR_INVALID_ARG
        assert len(r._l.atn_last_error(r._ctx)) > 10
        out = np.zeros((h, w), np.float32)
        assert r._l.atn_npr_shadow_download(r._ctx, 0, out.ctypes.data, out.size) == ERR_INVALID_ARG
        assert np.array_equal(r.render(w, h, 5, 3, frame=0), mode0)        # the bad values changed nothing
        assert r._l.atn_npr_shadow_download(r._ctx, 0, out.ctypes.data, out.size) == ERR_INVALID_ARG       # a mode-0 frame ran no pre-pass
        r.set_npr_shadow(1)
        r.render(w, h, 5, 3, frame=0, download=False)
        assert r._l.atn_npr_shadow_download(r._ctx, 0, out.ctypes.data, out.size - 1) == ERR_INVALID_ARG
        assert r._l.atn_npr_shadow_download(r._ctx, 3, out.ctypes.data, out.size) == ERR_INVALID_ARG
        assert r._l.atn_npr_shadow_download(r._ctx, 0, out.ctypes.data, out.size) == 0
        d = Destination(w, h, 5, 3, 1, 0, 1, 1, 1, 0)       # count_stats
        assert r._l.atn_render(r._ctx, C.byref(d), None) == ERR_UNSUPPORTED
    finally:
        r.close()
