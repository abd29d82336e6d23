"""The NPR look-through on the GPU (atn_npr_set_skip_through, device/npr_advance.hpp) against the CPU restatement of AdvanceNPRPath
(tests/cxx/npr_advance_oracle.cpp): stage parity, frame parity, byte-equality rules, scene edits, the refusals."""
import os

import numpy as np
import pytest

from conftest import make_camera, parity_record

pytestmark = pytest.mark.gpu

ERR_INVALID_ARG, ERR_UNSUPPORTED = -1, -5     # include/aten_amd.h


@pytest.fixture(scope="module")
def aq():
    import npr_advance_oracle
    npr_advance_oracle.lib()
    return npr_advance_oracle


@pytest.fixture(scope="module")
def rooms():
    import npr_advance_scenes as S
    return {k: make() for k, make in S.ROOMS.items()}


def _ctx(scene, cam, w, h, mode=1, env=None):
    from aten_amd.renderer import PathTracing
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        r = PathTracing(0)
        r.UpdateSceneData(scene)
    finally:
        for k, v in old.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = v
    r.updateCamera(cam)
    r.initSampler(w, h, 0)
    r.npr_set_skip_through(mode)
    return r


def _bytes(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("room", ["alpha", "stencil"])
def test_stage_parity(gpu, aq, orc, rooms, room):
    """Frames 0-3 at 64 x 48, depth 3.  On pixels whose disc after bounce 0 agrees: the look-through's stage (the check that said true,
    walks, answer, is_singular, transmission, throughput), the sample rays' live bits and the CMJ dimension, all exact.  The twin's
    stage holds every category the scenes were built for."""
    import npr_advance_scenes as S
    (fs, cam), names = rooms[room]
    w, h = 64, 48
    c = make_camera(orc, cam, w, h)
    seeds = orc.init_sampler(w, h, 0)
    r, o = _ctx(fs, c, w, h), aq.NPRAdvance()
    r.npr_capture(True)
    try:
        for f in range(4):
            got = r.npr_render(w, h, max_depth=3, frame=f)
            want, st = o.render(fs, c, seeds, w, h, max_depth=3, frame=f, stages=True)
            counts = S.category_counts(room, st["adv"])
            assert counts and all(v >= S.FLOOR for v in counts.values()), (f, counts)
            gd, wd = r.npr_buffer("disc"), st["disc"]
            same = np.all(gd["center"] == wd["center"], -1) & np.all(gd["normal"] == wd["normal"], -1) & (gd["radius"] == wd["radius"]) \
                & (gd["acc"] == wd["acc"])
            ga, wa = r.npr_advance_buffer(), st["adv"]
            gdesc, wdesc = r.npr_buffer("desc"), st["desc"]
            rates = {"disc": float(same.mean()),
                     "live": float(np.all(gdesc["live"] == wdesc["live"], -1)[same].mean()),
                     "dims": float((r.npr_buffer("dims") == st["dims"])[same & ~st["terminated"]].mean())}
            for k in ("kind", "walks", "answer", "singular", "transmission"):
                rates[k] = float((ga[k] == wa[k])[same].mean())
            rates["throughput"] = float(np.all(ga["throughput"] == wa["throughput"], -1)[same].mean())
            parity_record("NPR look-through stages, %s room 64x48, frame %d" % (room, f), got, want, tol=1e-3, stage_agreement=rates,
                          categories=counts)
            assert rates["disc"] >= 0.99, rates
            for k in ("kind", "walks", "answer", "singular", "transmission", "throughput", "live", "dims"):
                assert rates[k] == 1.0, (f, k, rates)
    finally:
        r.close(); o.close()


FRAME_CASES = [(room, spp, bt) for room in ("alpha", "stencil") for spp in (1, 4) for bt in (True, False)]
# Floors of the fraction of pixels within the frame tolerance, 0.2 percentage points under the first
# measurement (profiles/parity_npr_advance.jsonl): 100 % of pixels in every case and frame of both rooms -- analytic rooms, the
# npr_room class
FLOOR = {"alpha": 0.998, "stencil": 0.998}


@pytest.mark.parametrize("room,spp,brk", FRAME_CASES)
def test_frame_parity(gpu, aq, orc, rooms, room, spp, brk):
    (fs, cam), _ = rooms[room]
    w, h = 128, 72
    c = make_camera(orc, cam, w, h)
    seeds = orc.init_sampler(w, h, 0)
    r, o = _ctx(fs, c, w, h), aq.NPRAdvance()
    try:
        for f in range(5):
            got = r.npr_render(w, h, spp=spp, frame=f, break_on_terminate=brk)
            want = o.render(fs, c, seeds, w, h, spp=spp, frame=f, break_on_terminate=brk)
            m = parity_record("NPR look-through frame, %s room 128x72 spp %d break %d, frame %d" % (room, spp, int(brk), f), got, want)
            assert m["frac_within_0.001"] >= FLOOR[room], m
    finally:
        r.close(); o.close()


def _frames(scene, c, w, h, n=4, fif=1, mode=1, env=None, depth=5):
    r = _ctx(scene, c, w, h, mode=mode, env=env)
    try:
        if fif > 1:
            r.set_frames_in_flight(fif)
        for f in range(n):
            r.npr_render(w, h, max_depth=depth, frame=f, download=False)
        r.synchronize()
        return r.download_film()
    finally:
        r.close()


@pytest.mark.parametrize("which", ["npr_room", "npr_sponza"])
def test_mode_1_without_work_is_mode_0(gpu, orc, which):
    """A scene that needs no look-through: mode 1 launches nothing new, the film is mode 0's byte for byte."""
    from aten_amd.scene import scenedefs
    fs, cam = getattr(scenedefs, which)()
    w, h = 96, 54
    c = make_camera(orc, cam, w, h)
    assert _bytes(_frames(fs, c, w, h, mode=0), _frames(fs, c, w, h, mode=1))


@pytest.mark.parametrize("room", ["alpha", "stencil"])
def test_byte_equality(gpu, orc, rooms, room):
    (fs, cam), _ = rooms[room]
    w, h = 96, 54
    c = make_camera(orc, cam, w, h)
    one = _frames(fs, c, w, h)
    assert one[..., 3].max() == 4.0
    assert _bytes(one, _frames(fs, c, w, h)), "two identical runs"
    assert _bytes(one, _frames(fs, c, w, h, fif=4)), "4 frames in flight"
    assert _bytes(_frames(fs, c, w, h, env={"ATEN_AMD_TRACE": "r"}), _frames(fs, c, w, h, env={"ATEN_AMD_TRACE": "s"})), "refill / plain walk"
    assert _bytes(_frames(fs, c, w, h, env={"ATEN_AMD_LDS_NODES": "1"}), _frames(fs, c, w, h, env={"ATEN_AMD_LDS_NODES": "0"})), "LDS node walk on / off"
    assert _bytes(one, _frames(fs, c, w, h, env={"ATEN_AMD_TRACE": "s", "ATEN_AMD_LDS_NODES": "0"})), "the plain walk from global memory"
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
        # atn_render before and after look-through frames in one context
        before = r.render(w, h, frame=0, progressive=False)
        for f in range(2):
            r.npr_render(w, h, frame=f, download=False)
        after = r.render(w, h, frame=0, progressive=False)
    finally:
        r.close()
    assert _bytes(a, b), "npr_reset"
    assert _bytes(before, after), "atn_render around look-through frames"


def _refused(r, w, h, status=ERR_UNSUPPORTED, needle=None, **kw):
    with pytest.raises(Exception) as e:
        r.npr_render(w, h, **kw)
    assert "(status %d)" % status in str(e.value), str(e.value)
    if needle:
        assert needle in str(e.value), str(e.value)


@pytest.mark.parametrize("edit", ["alpha", "stencil"])
def test_material_edit(gpu, orc, edit):
    """atn_update_materials under mode 1: a material's alpha becomes 0.5 / its stencil type STENCIL -- the film of a context that
    uploaded the edited scene, byte for byte.  Under mode 0 the same context refuses the edited scene."""
    import npr_advance_scenes as S
    w, h = 96, 54
    name = "pane" if edit == "alpha" else "hair_front"

    def scene(edited):
        (fs, cam), names = S.ROOMS[edit]()
        m = fs.arrays["materials"]
        if not edited:
            if edit == "alpha": m["baseColor"][names[name]][3] = 1.0
            else: m["stencil_type"][names[name]] = 0
        return fs, cam, names

    fs0, cam, names = scene(False)
    fs1, _, _ = scene(True)
    c = make_camera(orc, cam, w, h)
    want = _frames(fs1, c, w, h, n=2)
    assert not _bytes(want, _frames(fs0, c, w, h, n=2)), "the edit changes the film"
    r = _ctx(fs0, c, w, h)
    try:
        r.npr_render(w, h, frame=0, download=False)         # (a frame of the scene as uploaded)
        r.updateMaterial(fs1, names[name], 1)
        r.npr_reset()
        for f in range(2):
            r.npr_render(w, h, frame=f, download=False)
        r.synchronize()
        assert _bytes(r.download_film(), want)
        r.npr_set_skip_through(0)
        _refused(r, w, h, needle="AdvanceNPRPath")
    finally:
        r.close()


def test_edit_into_the_look_through(gpu, orc):
    """A context that uploaded a scene with nothing to look through (npr_room) and runs mode 1: an edit that makes a material STENCIL
    is refused under mode 0 and rendered under mode 1, as the upload of the edited scene is."""
    from aten_amd.scene import scenedefs
    w, h = 64, 48
    fs, cam = scenedefs.npr_room()
    c = make_camera(orc, cam, w, h)
    r = _ctx(fs, c, w, h, mode=0)
    try:
        r.npr_render(w, h, frame=0, download=False)
        fs.arrays["materials"]["stencil_type"][1] = 2
        r.updateMaterial(fs, 1, 1)
        _refused(r, w, h, needle="StencilType::STENCIL")
        r.npr_set_skip_through(1)
        r.npr_reset()
        got = r.npr_render(w, h, frame=0)
    finally:
        r.close()
    assert _bytes(got, _frames(fs, c, w, h, n=1))


def test_refusals(gpu, orc, rooms):
    (fs, cam), _ = rooms["stencil"]
    (fa, _), _ = rooms["alpha"]
    w, h = 32, 24
    c = make_camera(orc, cam, w, h)
    for scene in (fs, fa):
        r = _ctx(scene, c, w, h, mode=0)
        try:
            _refused(r, w, h, needle="AdvanceNPRPath")                     # mode 0: today's refusals, with their messages
            with pytest.raises(Exception) as e:
                r.npr_set_skip_through(2)
            assert "(status %d)" % ERR_INVALID_ARG in str(e.value)
            with pytest.raises(Exception) as e:
                r.npr_set_skip_through(-1)
            assert "(status %d)" % ERR_INVALID_ARG in str(e.value)
            r.npr_set_skip_through(1)
            r.npr_render(w, h, frame=0)
            # the shadow pre-pass and the hatching modes on a scene that looks through something
            r.set_npr_shadow(1)
            _refused(r, w, h, needle="shadow pre-pass")
            r.set_npr_hatching(base="ao", direction=4, ao_num_rays=2, ao_radius=1.0)
            _refused(r, w, h, needle="hatching")
            r.set_npr_hatching(base=1, direction=1)
            r.set_npr_shadow(0)
            r.npr_render(w, h, frame=1)
            # no stage without capture
            with pytest.raises(Exception) as e:
                r.npr_advance_buffer()
            assert "(status %d)" % ERR_INVALID_ARG in str(e.value)
            # the other refusals are as they were
            r.set_shade_math(True)
            _refused(r, w, h)
            r.set_shade_math(False)
            r.setScreenShard(0, 2)
            _refused(r, w, h)
        finally:
            r.close()
    # a scene without look-through under mode 1: the pre-pass runs as ever
    from aten_amd.scene import scenedefs
    room, rcam = scenedefs.npr_room()
    r = _ctx(room, make_camera(orc, rcam, w, h), w, h, mode=1)
    try:
        r.set_npr_shadow(1)
        r.npr_render(w, h, frame=0)
    finally:
        r.close()
