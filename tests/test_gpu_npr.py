"""NPR feature lines on the GPU (atn_npr_*, device/npr.hpp) against the CPU restatement of the reference (tests/cxx/npr_oracle.cpp):
stage parity, frame parity, byte-equality rules and the refused configurations."""
import numpy as np
import pytest

from conftest import make_camera, parity_record

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nq():
    import npr_oracle
    npr_oracle.lib()
    return npr_oracle


@pytest.fixture(scope="module")
def room():
    from aten_amd.scene import scenedefs
    return scenedefs.npr_room()


@pytest.fixture(scope="module")
def sponza_npr():
    from aten_amd.scene import scenedefs
    return scenedefs.npr_sponza()


def _ctx(scene, cam, w, h):
    from aten_amd.renderer import PathTracing
    r = PathTracing(0)
    r.UpdateSceneData(scene)
    r.updateCamera(cam)
    r.initSampler(w, h, 0)
    return r


def _pair(nq, orc, scene, w, h):
    fs, cam = scene
    c = make_camera(orc, cam, w, h)
    return _ctx(fs, c, w, h), nq.NPR(), c, orc.init_sampler(w, h, 0)


@pytest.mark.parametrize("which", ["room", "sponza"])
def test_stage_parity(gpu, nq, orc, room, sponza_npr, which):
    """Frames 0-3: the disc draws u, v exact everywhere; on pixels whose disc after bounce 0 agrees (the same primary hit): the sample
    rays' live bits exact, the line decision (found, bounce) exact at bounce 0 and its distance within 1e-5 relative, and the CMJ dimension after
    bounce 0 exact where the path goes on (a path that ends at a first-hit toon surface is not shaded further here, while the
    reference's shade still draws its NEE and BSDF dimensions: unobservable, kernels.hpp)."""
    scene = room if which == "room" else sponza_npr
    w, h = (64, 48) if which == "room" else (96, 54)
    r, o, c, seeds = _pair(nq, orc, scene, w, h)
    r.npr_capture(True)
    try:
        for f in range(4):
            got = r.npr_render(w, h, max_depth=3, frame=f)
            want, st = o.render(scene[0], c, seeds, w, h, max_depth=3, frame=f, stages=True)
            gd, wd = r.npr_buffer("disc"), st["disc"]
            same = np.all(gd["center"] == wd["center"], -1) & np.all(gd["normal"] == wd["normal"], -1) & (gd["radius"] == wd["radius"]) \
                & (gd["acc"] == wd["acc"])
            gdesc, wdesc = r.npr_buffer("desc"), st["desc"]
            gl, wl = r.npr_buffer("line"), st["line"]
            dec = (gl["found"] == wl["found"]) & (~wl["found"] | (gl["bounce"] == wl["bounce"]))
            both = same & gl["found"] & wl["found"] & (gl["bounce"] == wl["bounce"])
            dist_ok = np.abs(gl["distance"] - wl["distance"]) <= 1e-5 * np.abs(wl["distance"])
            b0 = same & (wl["found"] & (wl["bounce"] == 0) | gl["found"] & (gl["bounce"] == 0))
            both0 = both & (wl["bounce"] == 0)
            rates = {"disc": float(same.mean()),
                     "uv": float((np.all(gdesc["u"] == wdesc["u"], -1) & np.all(gdesc["v"] == wdesc["v"], -1)).mean()),
                     "live": float(np.all(gdesc["live"] == wdesc["live"], -1)[same].mean()),
                     "dims": float((r.npr_buffer("dims") == st["dims"])[same & ~st["terminated"]].mean()),
                     "line": float(dec[same].mean()),
                     "line_bounce0": float(dec[b0].mean()) if b0.any() else 1.0,
                     "distance0": float(dist_ok[both0].mean()) if both0.any() else 1.0,
                     "distance": float(dist_ok[both].mean()) if both.any() else 1.0,
                     "lines": int(wl["found"].sum())}
            parity_record("NPR stages, %s %dx%d, frame %d" % (which, w, h, f), got, want, tol=1e-3, stage_agreement=rates)
            assert rates["lines"] > 0
            assert rates["disc"] >= 0.99, rates
            for k in ("uv", "live", "dims", "line_bounce0", "distance0"):
                assert rates[k] == 1.0, (f, k, rates)
            # a line found deeper in a path follows that path's own ulp divergences in the bounces before it (the path tracer's: the
            # frame test counts them); first measurement on sponza 99.96 % (decision) and 99.6 % (distance), the room 100 %
            assert rates["line"] >= 0.995 and rates["distance"] >= 0.99, rates
    finally:
        r.close(); o.close()


ERR_UNSUPPORTED = -5     # include/aten_amd.h

FRAME_CASES = [(s, spp, bt) for s in ("room", "sponza") for spp in (1, 4) for bt in (True, False)]
# Floors of the fraction of pixels within the frame tolerance, a small margin below the first measurement
# (profiles/parity_npr.jsonl): the room 100 % in every case, sponza 99.73-99.95 % (the path tracer's own ulp divergences behind the
# primary hit, and the lines found there)
FLOOR = {"room": 0.998, "sponza": 0.995}


@pytest.mark.parametrize("which,spp,brk", FRAME_CASES)
def test_frame_parity(gpu, nq, orc, room, sponza_npr, which, spp, brk):
    scene = room if which == "room" else sponza_npr
    w, h = 256, 144
    r, o, c, seeds = _pair(nq, orc, scene, w, h)
    try:
        for f in range(5):
            got = r.npr_render(w, h, spp=spp, frame=f, break_on_terminate=brk)
            want = o.render(scene[0], c, seeds, w, h, spp=spp, frame=f, break_on_terminate=brk)
            m = parity_record("NPR frame, %s 256x144 spp %d break %d, frame %d" % (which, spp, int(brk), f), got, want)
            assert m["frac_within_0.001"] >= FLOOR[which], m
    finally:
        r.close(); o.close()


def test_lines_on_no_material(gpu, nq, orc):
    """Lines on in the config, on no material: every query hit returns early, misses still trace their sample rays; the frame
    matches the twin (the 8 disc draws shift the sample stream, so it is not atn_render's frame)."""
    from aten_amd.scene import scenedefs
    scene = scenedefs.with_feature_lines(scenedefs.toon_room(), materials=[])
    w, h = 96, 72
    r, o, c, seeds = _pair(nq, orc, scene, w, h)
    try:
        for f in range(2):
            got = r.npr_render(w, h, frame=f)
            want = o.render(scene[0], c, seeds, w, h, frame=f)
            m = parity_record("NPR frame, lines on no material 96x72, frame %d" % f, got, want)
            assert m["frac_within_0.001"] >= 0.99, m
        pt = _ctx(scene[0], c, w, h)
        try:
            plain = pt.render(w, h, frame=0, progressive=False)
        finally:
            pt.close()
        first = _ctx(scene[0], c, w, h)
        try:
            assert not np.array_equal(first.npr_render(w, h, frame=0, progressive=False), plain)
        finally:
            first.close()
    finally:
        r.close(); o.close()


def _frames(scene, c, w, h, n=4, fif=1, spp=1, setup=None):
    r = _ctx(scene, c, w, h)
    try:
        if fif > 1:
            r.set_frames_in_flight(fif)
        if setup:
            setup(r)
        for f in range(n):
            r.npr_render(w, h, spp=spp, frame=f, download=False)
        r.synchronize()
        return r.download_film()
    finally:
        r.close()


def test_byte_equality(gpu, orc, room, sponza_npr):
    fs, cam = sponza_npr
    w, h = 160, 96
    c = make_camera(orc, cam, w, h)
    one = _frames(fs, c, w, h)
    assert np.array_equal(one, _frames(fs, c, w, h)), "two identical runs"
    assert np.array_equal(one, _frames(fs, c, w, h, fif=4)), "4 frames in flight"
    # npr_reset, then frame 0, against a fresh context
    r = _ctx(fs, c, w, h)
    try:
        for f in range(3):
            r.npr_render(w, h, frame=f, download=False)
        r.npr_reset()
        a = r.npr_render(w, h, frame=0)
    finally:
        r.close()
    r = _ctx(fs, c, w, h)
    try:
        b = r.npr_render(w, h, frame=0)
    finally:
        r.close()
    assert np.array_equal(a, b), "npr_reset"
    # atn_render before and after NPR frames in one context
    fr, rc = room
    c2 = make_camera(orc, rc, w, h)
    r = _ctx(fr, c2, w, h)
    try:
        before = r.render(w, h, frame=0, progressive=False)
        for f in range(2):
            r.npr_render(w, h, frame=f, download=False)
        after = r.render(w, h, frame=0, progressive=False)
    finally:
        r.close()
    assert np.array_equal(before, after), "atn_render around NPR frames"


def test_refused(gpu, orc, room):
    from aten_amd import layout as L
    from aten_amd.scene import scenedefs
    from aten_amd.renderer import PathTracing
    w, h = 32, 24
    fs, cam = room
    c = make_camera(orc, cam, w, h)

    def refused(scene, setup=None, **kw):
        r = PathTracing(0)
        try:
            r.UpdateSceneData(scene)
            r.updateCamera(c)
            r.initSampler(w, h, 0)
            if setup:
                setup(r)
            with pytest.raises(Exception) as e:
                r.npr_render(w, h, **kw)
            assert "(status %d)" % ERR_UNSUPPORTED in str(e.value), str(e.value)
        finally:
            r.close()

    refused(scenedefs.toon_room()[0])                                                  # feature lines off in the config
    refused(fs, setup=lambda r: r.setScreenShard(0, 2))
    refused(fs, setup=lambda r: r.set_regeneration(True), spp=2)
    refused(fs, setup=lambda r: r.set_shade_math(True))
    from aten_amd.renderer import Destination
    import ctypes as C
    r = _ctx(fs, c, w, h)
    try:
        d = Destination(w, h, 5, 3, 1, 0, 1, 1, 1, 0)                                 # count_stats
        assert r._l.atn_npr_render(r._ctx, C.byref(d), None) == ERR_UNSUPPORTED
    finally:
        r.close()
    stencil = scenedefs.npr_room()
    stencil[0].arrays["materials"]["stencil_type"][1] = 2
    refused(stencil[0])
    alpha = scenedefs.with_feature_lines(scenedefs.toon_room(alpha_blocker=True))
    refused(alpha[0])
    car = scenedefs.with_feature_lines(scenedefs.cornell_box_variant(extra_materials="carpaint"))
    assert (car[0].arrays["materials"]["type"] == L.MTRL_CARPAINT).any()
    refused(car[0])
