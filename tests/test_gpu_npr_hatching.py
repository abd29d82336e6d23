"""NPR hatching shadows on the GPU (atn_npr_hatching_*, device/npr_hatching.hpp) against the CPU twins (tests/cxx/
npr_hatching_oracle.cpp for the filters, the AO twin for the AO base's source plane, the NPR shadow twin for the bit and the depth):
the six filter directions as a stage, the AO source plane against the AO renderer itself, the frames that read the plane, the test
that fails without the feature, the byte-equality rules and the refusals.  docs/NPR_HATCHING.md has the decisions and the numbers."""
import numpy as np
import pytest

from conftest import make_camera, parity_record
from test_gpu_parity import frame_tolerance_report

pytestmark = pytest.mark.gpu

W, H = 100, 52
FRAMES = (0, 3)
ERR_INVALID_ARG, ERR_UNSUPPORTED = -1, -5     # include/aten_amd.h
# One step: the existing filter bound (docs/NPR_SHADOW.md "Parity": two expf that differ by <= ~2 ulp per weight, eleven-term sums and
# a division, <= ~32 * 2^-24 ~ 2e-6, doubled).  Two steps: a product of two values <= 1 each inside 4e-6 (<= 8e-6 + rounding); the
# halving is exact.
STEP_TOL, TWO_STEP_TOL = 4e-6, 1e-5
FLIP_CAP = 0.005        # at most this share of a plane may lie where the halving threshold can flip (product in [1 - 1e-5, 1))
AO_TOL, AO_FLOOR = 1e-3, 0.995      # tests/test_gpu_ao.py's bounds for the value plane
NONE, HORIZONTAL, VERTICAL, ORTHOGONAL, CROSS, ORTHOGONAL_CROSS = range(6)
AO, SHADOW_RAY = 0, 1
SETTINGS = [(SHADOW_RAY, CROSS, 1), (AO, HORIZONTAL, 4), (AO, ORTHOGONAL_CROSS, 4)]      # (base, direction, AO rays)


@pytest.fixture(scope="module")
def hq():
    import npr_hatching_oracle
    npr_hatching_oracle.lib()
    return npr_hatching_oracle


@pytest.fixture(scope="module")
def room(orc):
    """stylized_shadow_room, its camera and seeds at a size: computed once and shared."""
    from aten_amd.scene import scenedefs
    fs, cam = scenedefs.stylized_shadow_room()
    made = {}

    def get(w=W, h=H):
        if (w, h) not in made:
            made[(w, h)] = dict(fs=fs, c=make_camera(orc, cam, w, h), seeds=orc.init_sampler(w, h, 0))
        return made[(w, h)]
    return get


@pytest.fixture(scope="module")
def twin(orc, hq, room):
    """The twins' pre-pass per (size, frame, base, direction, rays), computed once and shared; the shadow twin's planes and the AO
    twin's value plane are shared between the directions.  Each result also has `toon` (the primary hit is a Toon / Stylized material)."""
    import npr_shadow_oracle
    from aten_amd import layout as L
    shadow, source, cache = {}, {}, {}

    def get(frame, base=SHADOW_RAY, direction=HORIZONTAL, rays=1, w=W, h=H):
        rm = room(w, h)
        if (w, h, frame) not in shadow:
            shadow[(w, h, frame)] = npr_shadow_oracle.prepass(rm["fs"], rm["c"], rm["seeds"], w, h, frame=frame)
        sp = shadow[(w, h, frame)]
        skey = (w, h, frame, base, rays if base == AO else 0)
        if skey not in source:
            source[skey] = hq.prepass(rm["fs"], rm["c"], rm["seeds"], w, h, frame=frame, base=base, direction=NONE, num_rays=rays, radius=1.0,
                                      shadow=sp)["source"]
        key = skey + (direction,)
        if key not in cache:
            plane, first = hq.filter(source[skey], sp["depth"], direction, first=True)
            mtrl = sp["mtrl"]
            toon = (mtrl >= 0) & np.isin(rm["fs"].arrays["materials"]["type"][mtrl.clip(0)], (L.MTRL_TOON, L.MTRL_STYLIZED))
            cache[key] = dict(source=source[skey], depth=sp["depth"], first=first, plane=plane, toon=toon)
        return cache[key]
    return get


def _ctx(rm, w=W, h=H, mode=1, setting=None):
    from aten_amd.renderer import PathTracing
    r = PathTracing(0)
    r.UpdateSceneData(rm["fs"])
    r.updateCamera(rm["c"])
    r.initSampler(w, h, 0)
    r.set_npr_shadow(mode)
    if setting is not None:
        r.set_npr_hatching(setting[0], setting[1], setting[2], 1.0)
    return r


def _plugged(plane):
    """A scene of its own for the CPU frame reference, the plane in its screen_space_texture."""
    import npr_shadow_oracle
    from aten_amd.scene import scenedefs
    fs, _ = scenedefs.stylized_shadow_room()
    return npr_shadow_oracle.plug_plane(fs, plane)


def _check_filtered(hq, name, direction, got, src, depth):
    """One direction's plane against the twin, every pixel -> the largest error outside the flip class."""
    want = hq.filter(src, depth, direction)
    miss = np.isinf(depth)
    if direction == NONE:
        assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(src, np.float32).view(np.uint32)), name
        return 0.0
    assert np.all(got[miss] == 1.0) and np.all(want[miss] == 1.0), (name, direction)
    two_step = direction in (CROSS, ORTHOGONAL_CROSS)
    tol = TWO_STEP_TOL if two_step else STEP_TOL
    # where the twin's product lies in [1 - 1e-5, 1) the halving may flip: checked on the twin to be rare before it is relied on
    flip = hq.flip_class(src, depth, direction)
    assert flip.mean() <= FLIP_CAP, (name, direction, flip.mean())
    g, w = got.astype(np.float64), want.astype(np.float64)
    err = np.abs(g - w)
    ok = err <= tol
    ok |= flip & (np.abs(g - 2.0 * w) <= tol)       # the twin halved (its product < 1), the device did not
    sure = ~flip
    worst = float(err[sure].max()) if sure.any() else 0.0
    print("hatching filter, %s direction %d: max |gpu - twin| = %.3g (bound %g), %d pixels in the flip class, %d miss-centred"
          % (name, direction, worst, tol, flip.sum(), miss.sum()))
    assert ok.all(), (name, direction, float(err[~ok].max()))
    return worst


# ---- 1. the filter as a stage
def test_filter_stage(gpu, hq, twin):
    inf = np.float32(np.inf)
    rng = np.random.default_rng(11)
    cases = []
    for w, h in ((112, 112), (100, 52)):
        t = twin(0, w=w, h=h)
        cases.append(("room lit %dx%d" % (w, h), t["source"], t["depth"]))
    t = twin(0, base=AO, rays=4)
    cases.append(("room AO %dx%d" % (W, H), t["source"], t["depth"]))
    for w, h in ((13, 3), (7, 2), (1, 1), (37, 4)):
        src = (rng.uniform(size=(h, w)) < 0.5).astype(np.float32)
        depth = rng.uniform(1.0, 1.5, (h, w)).astype(np.float32)
        depth[rng.uniform(size=(h, w)) < 0.25] = inf
        if (w, h) == (1, 1):
            depth[0, 0] = inf
        src[np.isinf(depth)] = 0.0
        cases.append(("synthetic %dx%d" % (w, h), src, depth))
    cases.append(("synthetic 1x1 hit", np.float32([[1.0]]), np.float32([[2.5]])))
    cases.append(("synthetic values 4x2", np.float32([[0.0, 1.7, 0.25, 1.0], [1.0, 0.5, 0.999, 1.7]]),
                  np.float32([[1.0, inf, 2.0, 1.0], [inf, 1.0, 1.0, 1.0]])))
    worst = {}
    for name, src, depth in cases:
        for direction in range(6):
            got = gpu.npr_hatching_filter(src, depth, direction)
            if direction != NONE and src.max() > 1.0:
                continue        # (AO values above 1 go through None as written; the clamped directions are tested on [0, 1] planes)
            e = _check_filtered(hq, name, direction, got, src, depth)
            worst[direction] = max(worst.get(direction, 0.0), e)
            if direction == HORIZONTAL:     # the row filter that exists, byte for byte
                assert np.array_equal(got.view(np.uint32), gpu.npr_shadow_filter(src, depth).view(np.uint32)), name
        parity_record("NPR hatching filter stage, %s" % name, gpu.npr_hatching_filter(src, depth, CROSS)[..., None].repeat(3, -1),
                      hq.filter(src, depth, CROSS)[..., None].repeat(3, -1), tol=TWO_STEP_TOL)
    print("hatching filter stage: worst per direction", worst)
    # all-lit: exactly 1 through every direction, not halved
    one = np.ones((9, 70), np.float32)
    for direction in range(6):
        assert np.array_equal(gpu.npr_hatching_filter(one, one * 2.0, direction), one), direction
    # sizes outside 1..16384, null planes and other directions are invalid arguments
    z = np.zeros((1, 1), np.float32)
    f = gpu._l.atn_npr_hatching_filter
    assert f(gpu._ctx, z.ctypes.data, z.ctypes.data, 0, 1, 1, z.ctypes.data) == ERR_INVALID_ARG
    assert f(gpu._ctx, z.ctypes.data, z.ctypes.data, 1, 16385, 1, z.ctypes.data) == ERR_INVALID_ARG
    assert f(gpu._ctx, None, z.ctypes.data, 1, 1, 1, z.ctypes.data) == ERR_INVALID_ARG
    assert f(gpu._ctx, z.ctypes.data, z.ctypes.data, 1, 1, 6, z.ctypes.data) == ERR_INVALID_ARG
    assert f(gpu._ctx, z.ctypes.data, z.ctypes.data, 1, 1, -1, z.ctypes.data) == ERR_INVALID_ARG


# ---- 2. the AO base's source plane
@pytest.mark.parametrize("rays", [1, 4])
def test_ao_source_plane(gpu, hq, twin, room, rays):
    """The source plane of a base-0 frame is the AO renderer's value plane on hit pixels, byte for byte: the same kernels over the same
    primary rays with the AO renderer's own sampler.  Misses are 1.0 / +inf.  Against the twin: the AO renderer's bounds."""
    rm = room()
    r = _ctx(rm, setting=(AO, HORIZONTAL, rays))
    a = _ctx(rm, mode=0)
    try:
        a.ao_set_params(rays, 1.0, False)
        for f in FRAMES:
            t = twin(f, base=AO, rays=rays)
            r.reset()
            r.render(W, H, 5, 3, frame=f, download=False)
            src, depth, plane = r.npr_hatching_buffer("source"), r.npr_shadow_buffer("depth"), r.npr_shadow_buffer("plane")
            a.ao_render(W, H, frame=f, break_on_terminate=False, download=False)
            value, adepth, state = a.ao_buffer("value"), a.ao_buffer("depth"), a.ao_buffer("state")
            hit = state == 1
            assert hit.sum() > 2000 and (~hit).sum() > 500
            assert np.array_equal(src[hit].view(np.uint32), value[hit].view(np.uint32))
            assert np.array_equal(depth[hit].view(np.uint32), adepth[hit].view(np.uint32))
            assert np.all(src[~hit] == 1.0) and np.all(np.isposinf(depth[~hit])) and np.all(plane[~hit] == 1.0)
            assert np.array_equal(depth.view(np.uint32), t["depth"].view(np.uint32))
            g, w = src.astype(np.float64), t["source"].astype(np.float64)
            within = np.abs(g - w) <= AO_TOL * np.maximum(1.0, np.abs(w))
            print("AO source plane, rays %d frame %d: byte-equal to the AO renderer on %d hit pixels; within %g of the twin on %.4f %%, "
                  "bit-equal %.4f %%" % (rays, f, hit.sum(), AO_TOL, 100 * within[hit].mean(), 100 * (src == t["source"])[hit].mean()))
            parity_record("NPR hatching AO source plane, rays %d frame %d" % (rays, f), src[..., None].repeat(3, -1),
                          t["source"][..., None].repeat(3, -1), tol=AO_TOL)
            assert within[hit].mean() >= AO_FLOOR
            # the row filter over it is the stage's
            assert np.array_equal(plane, gpu.npr_shadow_filter(src, depth))
            assert np.array_equal(r.npr_hatching_buffer("first"), plane)       # a one-step direction
            out = np.zeros((H, W), np.float32)
            assert r._l.atn_npr_shadow_download(r._ctx, 1, out.ctypes.data, out.size) == ERR_INVALID_ARG      # there is no bit
            assert b"lit bit" in r._l.atn_last_error(r._ctx)
    finally:
        r.close(); a.close()


# ---- 3. the frames that read the plane
@pytest.mark.parametrize("setting", SETTINGS, ids=["shadowray-cross", "ao-horizontal", "ao-orthogonalcross"])
def test_render_frames(gpu, orc, hq, twin, room, setting):
    base, direction, rays = setting
    rm = room()
    r = _ctx(rm, setting=setting)
    try:
        for f in FRAMES:
            t = twin(f, base=base, direction=direction, rays=rays)
            r.reset()
            got = r.render(W, H, 5, 3, frame=f)
            want = orc.render(_plugged(t["plane"]), rm["c"], rm["seeds"], W, H, 5, 3, frame=f)
            frac, mean_err = frame_tolerance_report(got, want)
            m = parity_record("NPR hatching frame, base %d direction %d rays %d %dx%d frame %d" % (base, direction, rays, W, H, f), got, want)
            print("atn_render mode 1, base %d direction %d, frame %d: within tolerance %.4f %%, mean err %.3g, max %.3g"
                  % (base, direction, f, 100 * frac, mean_err, m["max_abs_err"]))
            assert frac >= 0.995 and mean_err <= 5e-3, (frac, mean_err)
            # the planes behind the frame: the first step's and the final one against the twin where the sources agree
            src, first, plane = r.npr_hatching_buffer("source"), r.npr_hatching_buffer("first"), r.npr_shadow_buffer("plane")
            if direction in (CROSS, ORTHOGONAL_CROSS):
                want_first = hq.filter(src, t["depth"], HORIZONTAL if direction == CROSS else ORTHOGONAL)
                assert np.abs(first.astype(np.float64) - want_first).max() <= STEP_TOL
                assert not np.array_equal(first, plane)
            assert np.array_equal(plane, gpu.npr_hatching_filter(src, t["depth"], direction))
    finally:
        r.close()


def test_npr_render_runs_the_same_prepass(gpu, twin, room):
    """atn_npr_render (lines on) with {base 0, OrthogonalCross}: the planes of atn_render's pre-pass, byte for byte, and the frame
    against the NPR twin with the hatching twin's plane plugged in."""
    import npr_oracle
    import npr_shadow_oracle
    from aten_amd.scene import scenedefs
    setting, f = (AO, ORTHOGONAL_CROSS, 4), 3
    rm = room()
    t = twin(f, *setting)
    fs_lines, _ = scenedefs.with_feature_lines(scenedefs.stylized_shadow_room())
    a, b, o = _ctx(rm, setting=setting), _ctx(dict(rm, fs=fs_lines), setting=setting), npr_oracle.NPR()
    try:
        a.render(W, H, 5, 3, frame=f, download=False)
        got = b.npr_render(W, H, frame=f)
        for k in (0, 2):
            assert np.array_equal(a.npr_shadow_buffer(k).view(np.uint32), b.npr_shadow_buffer(k).view(np.uint32)), k
        for k in (0, 1):
            assert np.array_equal(a.npr_hatching_buffer(k).view(np.uint32), b.npr_hatching_buffer(k).view(np.uint32)), k
        fs_ref, _ = scenedefs.with_feature_lines((npr_shadow_oracle.plug_plane(scenedefs.stylized_shadow_room()[0], t["plane"]), None))
        want = o.render(fs_ref, rm["c"], rm["seeds"], W, H, frame=f)
        frac, mean_err = frame_tolerance_report(got, want)
        print("atn_npr_render mode 1, base 0 OrthogonalCross, frame %d: within tolerance %.4f %%, mean err %.3g" % (f, 100 * frac, mean_err))
        assert frac >= 0.995 and mean_err <= 5e-3, (frac, mean_err)
    finally:
        a.close(); b.close(); o.close()


# ---- 4. the test that fails without the feature
def test_cross_against_ao_on_the_toon_pixels_as_the_twin_says(gpu, orc, hq, twin, room):
    """On the toon pixels of frame 3 the Cross film (the lit bit) over the AO film (4 rays, the row filter) in sum is the ratio of the
    twin's two films, +- 2 %; non-toon pixels are byte-equal across all settings."""
    f = 3
    rm = room()
    t_cross, t_ao = twin(f, SHADOW_RAY, CROSS, 1), twin(f, AO, HORIZONTAL, 4)
    toon = t_cross["toon"]
    want_cross = orc.render(_plugged(t_cross["plane"]), rm["c"], rm["seeds"], W, H, 5, 3, frame=f)
    want_ao = orc.render(_plugged(t_ao["plane"]), rm["c"], rm["seeds"], W, H, 5, 3, frame=f)
    ratio_twin = float(want_cross[toon][:, :3].sum() / want_ao[toon][:, :3].sum())
    # (664 toon pixels at this size; the two films differ by more than the margin: the twin's ratio is 1.224)
    assert toon.sum() > 500 and abs(ratio_twin - 1.0) > 0.02, (toon.sum(), ratio_twin)
    films = {}
    for setting in [None] + SETTINGS:
        r = _ctx(rm, setting=setting)
        try:
            films[setting] = r.render(W, H, 5, 3, frame=f)
        finally:
            r.close()
    film_cross, film_ao = films[SETTINGS[0]], films[SETTINGS[1]]
    ratio_gpu = float(film_cross[toon][:, :3].sum() / film_ao[toon][:, :3].sum())
    print("toon pixels %d: Cross / AO in sum: gpu %.5f, twin %.5f" % (toon.sum(), ratio_gpu, ratio_twin))
    assert abs(ratio_gpu - ratio_twin) <= 0.02 * ratio_twin, (ratio_gpu, ratio_twin)
    for setting in SETTINGS:
        assert np.array_equal(films[None][~toon], films[setting][~toon]), setting      # nothing but toon shading reads the plane
        assert not np.array_equal(films[None][toon], films[setting][toon]), setting


# ---- 5. defaults and stability
def _run(rm, setting, in_flight=1, frames=6, mode=1, call_set=True):
    r = _ctx(rm, mode=mode, setting=setting if call_set else None)
    try:
        r.set_frames_in_flight(in_flight)
        for f in range(frames):
            r.render(W, H, 5, 3, frame=f, download=False)
        film = r.download_film()
        planes = [r.npr_shadow_buffer(k) for k in ((0, 2) if setting and setting[0] == AO else (0, 1, 2))] if mode == 1 else []
        if mode == 1:
            planes += [r.npr_hatching_buffer(0), r.npr_hatching_buffer(1)]
    finally:
        r.close()
    return film, planes


def _same(a, b):
    return np.array_equal(a[0], b[0]) and len(a[1]) == len(b[1]) and all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a[1], b[1]))


def test_defaults_and_stability(gpu, room):
    rm = room()
    # the defaults set explicitly are a context that never called the entry
    never = _run(rm, (SHADOW_RAY, HORIZONTAL, 1), call_set=False)
    assert _same(_run(rm, (SHADOW_RAY, HORIZONTAL, 1)), never)
    assert _same(_run(rm, (SHADOW_RAY, HORIZONTAL, 7)), never)      # the AO parameters are read with base 0 only
    # base 0: frames in flight, two runs
    for setting in ((AO, HORIZONTAL, 4), (AO, ORTHOGONAL_CROSS, 2), (SHADOW_RAY, CROSS, 1)):
        one = _run(rm, setting, 1)
        four = _run(rm, setting, 4)
        assert _same(one, four), setting
        assert _same(four, _run(rm, setting, 4)), setting
        assert not np.array_equal(one[0], never[0]), setting
    # the settings are context state: they survive an upload; mode 0 ignores them, and after base-0 frames it is a fresh context's
    fresh = _run(rm, None, mode=0)
    r = _ctx(rm, setting=(AO, CROSS, 3))
    try:
        r.set_npr_hatching(AO, CROSS, 3, 0.75)
        r.UpdateSceneData(rm["fs"])
        assert r.npr_hatching() == dict(base=AO, direction=CROSS, ao_num_rays=3, ao_radius=0.75)
        for f in range(3):
            r.render(W, H, 5, 3, frame=f, download=False)
        r.set_npr_shadow(0)
        r.reset()
        for f in range(6):
            r.render(W, H, 5, 3, frame=f, download=False)
        assert np.array_equal(r.download_film(), fresh[0])
    finally:
        r.close()


# ---- 6. refusals and bad arguments
def test_refused(gpu, room):
    import ctypes as C
    from aten_amd.renderer import Destination
    from aten_amd.scene import scenedefs
    rm = room()
    r0 = _ctx(rm, mode=0)
    try:
        mode0 = r0.render(W, H, 5, 3, frame=0)
        # bad arguments change nothing, before a pre-pass nothing can be downloaded
        r0.set_npr_hatching(AO, VERTICAL, 5, 0.5)
        before = r0.npr_hatching()
        for bad in ((-1, 1, 1, 1.0), (2, 1, 1, 1.0), (1, -1, 1, 1.0), (1, 6, 1, 1.0), (0, 1, 0, 1.0), (0, 1, 65, 1.0), (0, 1, 1, 0.0),
                    (0, 1, 1, -1.0), (0, 1, 1, float("inf")), (0, 1, 1, float("nan")), (1, 1, 0, 1.0)):
            assert r0._l.atn_npr_hatching_set(r0._ctx, *bad) == ERR_INVALID_ARG, bad
            assert len(r0._l.atn_last_error(r0._ctx)) > 10
            assert r0.npr_hatching() == before, bad
        out = np.zeros((H, W), np.float32)
        assert r0._l.atn_npr_hatching_download(r0._ctx, 0, out.ctypes.data, out.size) == ERR_INVALID_ARG
        r0.reset()
        assert np.array_equal(r0.render(W, H, 5, 3, frame=0), mode0)        # mode 0 ignores the settings
        r0.set_npr_shadow(1)
        r0.render(W, H, 5, 3, frame=0, download=False)
        assert r0._l.atn_npr_hatching_download(r0._ctx, 0, out.ctypes.data, out.size - 1) == ERR_INVALID_ARG
        assert r0._l.atn_npr_hatching_download(r0._ctx, 2, out.ctypes.data, out.size) == ERR_INVALID_ARG
        assert r0._l.atn_npr_hatching_download(r0._ctx, 0, out.ctypes.data, out.size) == 0
        assert r0._l.atn_npr_shadow_download(r0._ctx, 1, out.ctypes.data, out.size) == ERR_INVALID_ARG       # base 0: no bit
        assert r0._l.atn_npr_shadow_download(r0._ctx, 3, out.ctypes.data, out.size) == ERR_INVALID_ARG
        assert r0._l.atn_npr_shadow_download(r0._ctx, 0, out.ctypes.data, out.size) == 0
        # more than 2^28 listed AO rays: refused in front of the frame, nothing is allocated
        r0.set_npr_hatching(AO, VERTICAL, 64, 0.5)
        d = Destination(2049, 2048, 5, 3, 1, 0, 1, 1, 0, 0)
        assert r0._l.atn_render(r0._ctx, C.byref(d), None) == ERR_UNSUPPORTED
        assert b"2^28" in r0._l.atn_last_error(r0._ctx)
        r0.set_npr_shadow(0)
        r0.reset()
        assert np.array_equal(r0.render(W, H, 5, 3, frame=0), mode0)
    finally:
        r0.close()

    def refused(scene, setup, undo, call=None, expect=mode0, **kw):
        r = _ctx(dict(rm, fs=scene), setting=(AO, CROSS, 2))
        try:
            setup(r)
            with pytest.raises(Exception) as e:
                (call or (lambda q: q.render(W, H, 5, 3, frame=0, **kw)))(r)
            assert "(status %d)" % ERR_UNSUPPORTED in str(e.value), str(e.value)
            assert "NPR" in str(e.value) and len(str(e.value)) > len("(status -5)") + 10, str(e.value)
            undo(r)
            r.set_npr_shadow(0)
            r.reset()
            film = r.render(W, H, 5, 3, frame=0)
            if expect is not None:
                assert np.array_equal(film, expect)
        finally:
            r.close()

    nothing = lambda r: None
    refused(rm["fs"], lambda r: r.setScreenShard(0, 2), lambda r: r.setScreenShard(0, 1))
    refused(rm["fs"], lambda r: r.set_regeneration(True), lambda r: r.set_regeneration(False))
    refused(rm["fs"], nothing, nothing, call=lambda r: r.render_burst(W, H, 2, 5, 3, frame=0))
    refused(rm["fs"], lambda r: r.set_shade_math(True), lambda r: r.set_shade_math(False))
    refused(rm["fs"], nothing, nothing, count_stats=True)
    car = scenedefs.cornell_box_variant(extra_materials="carpaint")
    refused(car[0], nothing, nothing, expect=None)
