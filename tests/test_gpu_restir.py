"""ReSTIR on the GPU (atn_restir_*, device/restir.hpp) against the CPU restatement of the reference (tests/cxx/restir_oracle.cpp):
stage parity of the reservoirs, frame parity, the benefit of reuse, byte-equality rules and the refused configurations."""
import ctypes as C

import numpy as np
import pytest

from conftest import make_camera, parity_record

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rs():
    import restir_oracle
    restir_oracle.lib()
    return restir_oracle


@pytest.fixture(scope="module")
def ml_cornell():
    from aten_amd.scene import scenedefs
    return scenedefs.many_light_cornell(8)


@pytest.fixture(scope="module")
def ml_sponza():
    from aten_amd.scene import scenedefs
    return scenedefs.many_light_sponza()


def _ctx(gpu, scene, cam, w, h):
    from aten_amd.renderer import PathTracing
    r = PathTracing(0)
    r.UpdateSceneData(scene)
    r.updateCamera(cam)
    r.initSampler(w, h, 0)
    return r


def _pair(gpu, rs, orc, scene, w, h):
    fs, cam = scene
    c = make_camera(orc, cam, w, h)
    return _ctx(gpu, fs, c, w, h), rs.ReSTIR(), c, orc.init_sampler(w, h, 0)


def _same_hit(gi, oi):
    return (gi["mtrl"] == oi["mtrl"]) & (gi["mesh"] == oi["mesh"]) & np.all(gi["p"] == oi["p"], axis=-1) & (gi["hit"] == oi["hit"])


@pytest.mark.parametrize("which", ["cornell", "sponza", "cornell-37x21", "cornell-100x52"])
def test_stage_parity(gpu, rs, orc, ml_cornell, ml_sponza, which):
    """Reservoir y and M exact, W within 1e-4 relative after the initial, temporal and spatial passes, and the CMJ dimension after
    bounce 0, on pixels whose primary hit agrees -- four consecutive frames of mode 1 (frames 2 and 3 run the temporal pass).
    37 x 21 and 100 x 52: frames whose edges line up with no tile of the reuse passes."""
    scene = ml_sponza if which == "sponza" else ml_cornell
    w, h = tuple(int(v) for v in which.split("-")[1].split("x")) if "-" in which else (64, 48) if which == "cornell" else (96, 54)
    r, o, c, seeds = _pair(gpu, rs, orc, scene, w, h)
    r.restir_capture(True)
    r.restir_set_options(1, 8)
    # every pixel whose primary hit agrees agrees in every stage: the kernels run the oracle's operations in the oracle's order
    try:
        for f in range(4):
            got = r.restir_render(w, h, max_depth=3, frame=f, compute_motion=True)
            want, st = o.render(scene[0], c, seeds, w, h, max_depth=3, frame=f, mode=1, n_candidates=8, compute_motion=True, stages=True)
            gi = r.restir_buffer("info")
            same = _same_hit(gi, st["info"])
            rates = {"hit": float(same.mean())}
            live = same & ~st["terminated"]
            for k in ("initial", "temporal", "spatial"):
                g, wnt = r.restir_buffer(k), st[k]
                mask = same if k != "spatial" else live
                ok = (g["y"] == wnt["y"]) & (g["M"] == wnt["M"]) & (np.abs(g["W"] - wnt["W"]) <= 1e-4 * np.maximum(np.abs(wnt["W"]), 1e-30))
                rates[k] = float(ok[mask].mean())
            rates["dims"] = float((r.restir_buffer("dims") == st["dims"])[same].mean())
            parity_record("ReSTIR stages, many-light %s %dx%d mode 1, frame %d" % (which, w, h, f), got, want, tol=1e-3, stage_agreement=rates)
            for k, v in rates.items():
                assert v == 1.0, (f, k, rates)
    finally:
        r.close(); o.close()


FRAME_CASES = [(s, m, n) for s in ("cornell", "sponza") for m in (0, 1, 2, 3) for n in (1, 32)]
# Floors of the fraction of pixels within the frame tolerance, each a small margin below its first
# measurement (profiles/parity_restir.jsonl): Cornell 100 % in every mode, sponza 99.29-99.85 % in every mode (the pixels outside
# are the path tracer's own ulp divergences in the bounces behind the primary hit: the stage test is exact).
FLOOR = {"cornell": 0.995, "sponza": 0.99}


@pytest.mark.parametrize("which,mode,ncand", FRAME_CASES)
def test_frame_parity(gpu, rs, orc, ml_cornell, ml_sponza, which, mode, ncand):
    scene = ml_cornell if which == "cornell" else ml_sponza
    w, h = 256, 144
    r, o, c, seeds = _pair(gpu, rs, orc, scene, w, h)
    r.restir_set_options(mode, ncand)
    floor = FLOOR[which]
    try:
        for f in range(5):
            got = r.restir_render(w, h, frame=f, compute_motion=True)
            want = o.render(scene[0], c, seeds, w, h, frame=f, mode=mode, n_candidates=ncand, compute_motion=True)
            m = parity_record("ReSTIR frame, many-light %s 256x144 mode %d n_candidates %d, frame %d" % (which, mode, ncand, f), got, want)
            assert m["frac_within_0.001"] >= floor, m
    finally:
        r.close(); o.close()


def test_frame_parity_moving_camera_and_mixed_lights(gpu, rs, orc, ml_cornell):
    from aten_amd.scene import scenedefs
    w, h = 128, 72
    for scene, moving in ((ml_cornell, True), (scenedefs.cornell_box_variant("mixed"), False)):
        fs, cam = scene
        c0 = make_camera(orc, cam, w, h)
        r, o = _ctx(gpu, fs, c0, w, h), rs.ReSTIR()
        seeds = orc.init_sampler(w, h, 0)
        try:
            for f in range(5):
                pos = (cam["pos"][0] + (0.03 * f if moving else 0.0), cam["pos"][1], cam["pos"][2])
                c = orc.create_camera(pos, cam["at"], cam["vfov"], w, h)
                r.updateCamera(c)
                got = r.restir_render(w, h, frame=f, compute_motion=True)
                want = o.render(fs, c, seeds, w, h, frame=f, mode=1, n_candidates=32, compute_motion=True)
                m = parity_record("ReSTIR frame, %s 128x72 mode 1, frame %d" % ("moving camera" if moving else "mixed lights", f), got, want)
                assert m["frac_within_0.001"] >= 0.995, m        # (measured: 100 %)
            if moving:
                md = r.restir_buffer("motion")
                assert np.abs(md[..., 0]).max() > 0
        finally:
            r.close(); o.close()


def test_reuse_lowers_variance(gpu, orc, ml_sponza):
    """Direct light only (max_depth 1): the per-pixel variance over 16 frames of mode 1 (temporal + spatial reuse) is below that
    of mode 0 (32 initial candidates)"""
    fs, cam = ml_sponza
    w, h = 128, 72
    c = make_camera(orc, cam, w, h)
    var = {}
    for mode in (0, 1):
        r = _ctx(gpu, fs, c, w, h)
        r.restir_set_options(mode, 32)
        imgs = np.array([r.restir_render(w, h, max_depth=1, frame=f, compute_motion=True, progressive=False)[..., :3].sum(-1)
                         for f in range(16)])
        r.close()
        var[mode] = float(np.nanmean(imgs[4:].var(axis=0)))
    print("per-pixel variance over frames 4-15, mode 0 / mode 1:", var)
    assert var[1] < var[0], var


def test_direct_light_against_path_tracer(gpu, orc, ml_cornell):
    """Oracle-free: GPU mode 0 against the GPU path tracer's NEE at max_depth 1 on point lights, 32 frames, 8 x 8 blocks.  One-sided:
    the reference's visibility origin (p + AT_MATH_EPSILON * nml) lets some visibility rays hit their own surface, so ReSTIR may be
    darker, never brighter (tests/test_restir_oracle_cpu.py shows the two agree once the origin is moved off the surface)."""
    fs, cam = ml_cornell
    w, h = 64, 48
    c = make_camera(orc, cam, w, h)
    r = _ctx(gpu, fs, c, w, h)
    r.restir_set_options(0, 8)
    a, b = [], []
    for f in range(32):
        a.append(r.restir_render(w, h, max_depth=1, frame=f, compute_motion=True, progressive=False)[..., :3].sum(-1))
        b.append(r.render(w, h, max_depth=1, frame=f, progressive=False)[..., :3].sum(-1))
    r.close()
    a, b = np.array(a, np.float64), np.array(b, np.float64)
    z = []
    for y in range(0, h, 8):
        for x in range(0, w, 8):
            sa, sb = a[:, y:y + 8, x:x + 8].reshape(-1), b[:, y:y + 8, x:x + 8].reshape(-1)
            se = np.sqrt(sa.var(ddof=1) / len(sa) + sb.var(ddof=1) / len(sb))
            if se > 0:
                z.append((sa.mean() - sb.mean()) / se)
    z = np.array(z)
    assert len(z) > 20
    assert z.max() <= 4.0, z
    assert a.mean() <= b.mean()


def test_capture_and_motion_buffers(gpu, orc, ml_cornell):
    """Stage buffers are served only for a frame that kept them; compute_motion never overwrites the caller's motion buffer."""
    from aten_amd.renderer import AtenAmdError
    fs, cam = ml_cornell
    w, h = 64, 48
    c = make_camera(orc, cam, w, h)
    r = _ctx(gpu, fs, c, w, h)
    try:
        mine = np.full((h, w, 4), 0.0, np.float32)
        mine[..., 2] = 1.0
        mine[..., 3] = 1.0
        r.restir_set_motion_depth(mine)
        r.restir_render(w, h, frame=0, compute_motion=False)
        r.restir_capture(True)
        with pytest.raises(AtenAmdError, match="stage buffers"):
            r.restir_buffer("initial")
        assert r.restir_buffer("motion").tobytes() == mine.tobytes()
        r.restir_render(w, h, frame=1, compute_motion=True)
        r.restir_buffer("initial")
        assert r.restir_buffer("motion").tobytes() != mine.tobytes()        # the computed one (depth = clip w of the hits)
        r.restir_capture(False)
        r.restir_render(w, h, frame=2, compute_motion=False)
        assert r.restir_buffer("motion").tobytes() == mine.tobytes()
        with pytest.raises(AtenAmdError, match="stage buffers"):
            r.restir_buffer("spatial")
    finally:
        r.close()


def _frames(r, w, h, n, **kw):
    return [r.restir_render(w, h, frame=f, compute_motion=True, **kw).tobytes() for f in range(n)]


def test_byte_equality(gpu, orc, ml_cornell):
    fs, cam = ml_cornell
    w, h = 128, 72
    c = make_camera(orc, cam, w, h)
    a = _ctx(gpu, fs, c, w, h)
    ref = _frames(a, w, h, 4)
    a.restir_reset()
    a.reset()
    assert _frames(a, w, h, 1)[0] == ref[0]             # restir_reset, then frame 0 = a fresh context's frame 0
    a.close()
    b = _ctx(gpu, fs, c, w, h)
    assert _frames(b, w, h, 4) == ref                   # two identical runs
    b.close()
    d = _ctx(gpu, fs, c, w, h)
    d.set_frames_in_flight(4)
    got = [d.restir_render(w, h, frame=f, compute_motion=True, download=False) for f in range(3)]
    got.append(d.restir_render(w, h, frame=3, compute_motion=True))
    assert got[-1].tobytes() == ref[-1]                 # four frames in flight
    d.close()
    # atn_render gives the same bytes before and after ReSTIR frames in the same context
    e = _ctx(gpu, fs, c, w, h)
    before = e.render(w, h, frame=0, progressive=False).tobytes()
    _frames(e, w, h, 3)
    after = e.render(w, h, frame=0, progressive=False).tobytes()
    e.close()
    assert before == after


def test_unsupported(gpu, orc, ml_cornell):
    from aten_amd._lib import Destination
    from aten_amd.renderer import AtenAmdError
    fs, cam = ml_cornell
    w, h = 64, 48
    c = make_camera(orc, cam, w, h)
    r = _ctx(gpu, fs, c, w, h)
    try:
        d = Destination(w, h, 5, 3, 2, 0, 1, 1, 0, 0)
        assert r._l.atn_restir_render(r._ctx, C.byref(d), 1, None) == -5
        assert "sample" in r._l.atn_last_error(r._ctx).decode()
        d = Destination(w, h, 5, 3, 1, 0, 1, 1, 1, 0)
        assert r._l.atn_restir_render(r._ctx, C.byref(d), 1, None) == -5
        r.set_shade_math(True)
        with pytest.raises(AtenAmdError, match="relaxed"):
            r.restir_render(w, h, compute_motion=True)
        r.set_shade_math(False)
        r.set_regeneration(True)
        with pytest.raises(AtenAmdError, match="regeneration"):
            r.restir_render(w, h, compute_motion=True)
        r.set_regeneration(False)
        r.setScreenShard(0, 2)
        with pytest.raises(AtenAmdError, match="one GPU"):
            r.restir_render(w, h, compute_motion=True)
        r.setScreenShard(0, 1)
        with pytest.raises(AtenAmdError, match="motion"):
            r.restir_render(w, h, compute_motion=False)
        r.restir_render(w, h, compute_motion=True)
    finally:
        r.close()


def test_zero_lights(gpu, rs, orc, cornell):
    """A scene without lights: no candidates (M = 0), only what the bounces behind the primary hit find"""
    from aten_amd.scene import scenedefs
    fs, cam = scenedefs.cornell_box_variant("none", move_boxes=False)
    w, h = 64, 48
    r, o, c, seeds = _pair(gpu, rs, orc, (fs, cam), w, h)
    try:
        r.restir_capture(True)
        got = r.restir_render(w, h, frame=0, compute_motion=True)
        want, st = o.render(fs, c, seeds, w, h, frame=0, compute_motion=True, stages=True)
        assert np.all(r.restir_buffer("initial")["M"] == 0) and np.all(st["initial"]["M"] == 0)
        m = parity_record("ReSTIR frame, Cornell without lights 64x48", got, want)
        assert m["frac_within_0.001"] >= 0.99, m
    finally:
        r.close(); o.close()
