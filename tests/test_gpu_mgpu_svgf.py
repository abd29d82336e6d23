"""Node-wide SVGF (atn_mgpu_svgf_*, aten_amd/csrc/host/mgpu.hpp, docs/MGPU_SVGF.md): the path pass on every shard, the four hand-over
planes packed, pushed and unpacked onto shard 0, the filters there.  Contract: whatever the shard count, every result is BYTE-equal
to a fresh single PathTracing context given the same calls in the same order.  The shards of these tests share the box's one GPU
(an ordinal may repeat), which runs the whole N > 1 path: worker threads, screen shards, pack, copies, events, unpack.

Every case plays one script of calls on both sides (Cornell box, depth 5, a-trous iterations at the default) and compares what the
calls return with tobytes()."""
import numpy as np
import pytest

from aten_amd.scene.camera import create_camera

pytestmark = pytest.mark.gpu

SIZES = ((64, 48), (100, 52))       # 48 tiles; 91 tiles: ragged edge tiles, and 91 is not a multiple of 2, 3 or 8
GATHER_PLANES = ("contribs", "primary_position", "motion_depth",                   # which = 14, 10, 9
                 "prev_normal_depth", "prev_albedo_meshid", "prev_color_variance", "prev_moment_temporalweight")      # 4 - 7


def _camera(cam, w, h, step):
    """The fixture's camera moved sideways, up and forwards by `step` times a few centimetres (the room is two metres wide)."""
    pos = [cam["pos"][0] + 0.07 * step, cam["pos"][1] + 0.03 * step, cam["pos"][2] - 0.05 * step]
    return create_camera(pos, cam["at"], cam["vfov"], w, h)


def _play(r, fs, cam, script):
    """Plays `script` on a renderer (either class: the calls have the same names) and returns what its calls returned, as bytes."""
    got = []
    w = h = 0
    r.UpdateSceneData(fs)
    for op in script:
        if op[0] == "size":
            _, w, h = op
            r.initSampler(w, h, 0)
            r.updateCamera(_camera(cam, w, h, 0))
        elif op[0] == "cam":
            r.updateCamera(_camera(cam, w, h, op[1]))
        elif op[0] == "svgf":
            kw = dict(compute_motion=True, stages=True)
            kw.update(op[2])
            res = r.svgf_render(w, h, 5, 3, frame=op[1], **kw)
            if res is not None:
                got.extend(a.tobytes() for a in (res if isinstance(res, tuple) else (res,)))
        elif op[0] == "buf":
            got.append(r.svgf_buffer(op[1]).tobytes())
        elif op[0] == "render":
            got.append(r.render(w, h, 5, 3, frame=op[1]).tobytes())
        elif op[0] == "motion":
            r.svgf_set_motion_depth(op[1])
        elif op[0] == "reset":
            r.svgf_reset()
        elif op[0] == "in_flight":
            r.set_frames_in_flight(op[1])
        elif op[0] == "sync":
            r.synchronize()
        else:
            raise ValueError(op)
    return got


def _single(fs, cam, script):
    from aten_amd.renderer import PathTracing
    r = PathTracing(0)
    try:
        return _play(r, fs, cam, script)
    finally:
        r.close()


def _multi(devices, fs, cam, script):
    from aten_amd.renderer import MultiGpuPathTracing
    m = MultiGpuPathTracing(devices)
    try:
        return _play(m, fs, cam, script), m.shard_count()
    finally:
        m.close()


def _same(got, want, what):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, (what, "result %d of the script differs" % i)


# Four frames with computed motion; the camera moves between frames 1 -> 2 and 2 -> 3, so temporal reprojection sees non-zero motion.
# Every frame returns the output and the three stage planes; after frame 2 the planes the exchange fills (and what PrepareForDenoise
# made of them: the previous AOV set) are read back, which tells an exchange error from a filter-ordering error.
def _main_script(w, h):
    s = [("size", w, h), ("svgf", 0, {}), ("svgf", 1, {}), ("cam", 1), ("svgf", 2, {})]
    s += [("buf", name) for name in GATHER_PLANES]
    s += [("cam", 2), ("svgf", 3, {})]
    return s


N_FRAME_RESULTS = 2         # (out, stages) per frame
_runs = {}


def _main_run(cornell, size, shards):
    """The main script's results on `shards` shards sharing GPU 0 (0: one PathTracing context), played once per (size, shards)."""
    key = (size, shards)
    if key not in _runs:
        fs, cam = cornell
        if shards == 0:
            _runs[key] = _single(fs, cam, _main_script(*size))
        else:
            got, n = _multi([0] * shards, fs, cam, _main_script(*size))
            assert n == shards
            _runs[key] = got
    return _runs[key]


def _split(results):
    """(frame results, gather-plane results) of a main-script run"""
    k = 3 * N_FRAME_RESULTS
    return results[:k] + results[k + len(GATHER_PLANES):], results[k:k + len(GATHER_PLANES)]


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("shards", [1, 2, 3, 8])
def test_shards_equal_one_context(cornell, shards, size):
    """out_host and the three stages_host planes of every one of the four frames."""
    got, _ = _split(_main_run(cornell, size, shards))
    want, _ = _split(_main_run(cornell, size, 0))
    assert len(want) == 4 * N_FRAME_RESULTS
    _same(got, want, (shards, size))


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("shards", [1, 2, 3, 8])
def test_the_gather_alone(cornell, shards, size):
    """After frame 2: contributions (14), primary positions (10), motion/depth (9) and the previous-set AOVs (4 - 7) of shard 0
    against the single context's."""
    _, got = _split(_main_run(cornell, size, shards))
    _, want = _split(_main_run(cornell, size, 0))
    assert len(want) == len(GATHER_PLANES)
    for name, a, b in zip(GATHER_PLANES, got, want):
        assert a == b, (shards, size, name)


@pytest.mark.parametrize("shards,size", [(3, (1, 1)), (3, (5, 3)), (8, (8, 8))])
def test_tiny_frames(cornell, shards, size):
    """One tile (with three shards two of them own no tile at all; with eight, seven), three frames, the camera moving."""
    fs, cam = cornell
    script = [("size",) + size, ("svgf", 0, {}), ("svgf", 1, {}), ("cam", 1), ("svgf", 2, {}), ("buf", "contribs"), ("buf", "primary_position")]
    got, n = _multi([0] * shards, fs, cam, script)
    assert n == shards
    _same(got, _single(fs, cam, script), (shards, size))


def test_two_samples_per_pixel(cornell):
    fs, cam = cornell
    script = [("size", 64, 48), ("svgf", 0, dict(spp=2)), ("cam", 1), ("svgf", 1, dict(spp=2)), ("buf", "contribs")]
    got, _ = _multi([0, 0, 0], fs, cam, script)
    _same(got, _single(fs, cam, script), "spp = 2")


def test_callers_motion_depth_plane(cornell):
    """compute_motion = 0: the filters read the plane of atn_mgpu_svgf_set_motion_depth (it lives on shard 0)."""
    fs, cam = cornell
    w, h = 64, 48
    rng = np.random.default_rng(5)
    md = np.zeros((h, w, 4), np.float32)
    md[..., :2] = rng.uniform(-0.02, 0.02, (h, w, 2)).astype(np.float32)
    md[..., 2] = rng.uniform(1.0, 5.0, (h, w)).astype(np.float32)
    md[..., 3] = 1.0
    kw = dict(compute_motion=False)
    script = [("size", w, h), ("motion", md), ("svgf", 0, kw), ("svgf", 1, kw), ("cam", 1), ("svgf", 2, kw), ("buf", "motion_depth")]
    got, _ = _multi([0, 0], fs, cam, script)
    _same(got, _single(fs, cam, script), "caller's motion plane")


def test_frames_in_flight_then_one_download(cornell):
    """Three frames in flight on three shards, six frames with no host pointer: bank streams rotate, the packed and gather buffers and
    the hand-over slots are reused twice, and only events order any of it.  The single context runs one frame at a time."""
    fs, cam = cornell
    w, h = 100, 52
    frames = lambda kw: [("svgf", 0, kw), ("svgf", 1, kw), ("cam", 1), ("svgf", 2, kw), ("cam", 2), ("svgf", 3, kw), ("svgf", 4, kw),
                         ("cam", 3), ("svgf", 5, kw)]
    quiet = dict(stages=False, download=False)
    got, _ = _multi([0, 0, 0], fs, cam, [("size", w, h), ("in_flight", 3)] + frames(quiet) + [("sync",), ("buf", "output")])
    want = _single(fs, cam, [("size", w, h)] + frames(dict(stages=False)))
    assert len(got) == 1 and len(want) == 6
    assert got[0] == want[5]


def test_frames_in_flight_at_a_size_where_frames_overlap(cornell):
    """The same at 640x360 (3600 tiles) with four frames in flight on four shards: a frame's passes now take long enough for the next
    frames' path passes, packs and copies to run beside them, so a missing wait has something to race with.  Eight frames, the last
    one downloaded with its stage planes."""
    fs, cam = cornell
    w, h = 640, 360
    quiet = dict(stages=False, download=False)
    body = []
    for f in range(7):
        body += [("cam", f), ("svgf", f, quiet)]
    body += [("cam", 7), ("svgf", 7, {}), ("buf", "contribs"), ("buf", "prev_moment_temporalweight")]
    got, _ = _multi([0, 0, 0, 0], fs, cam, [("size", w, h), ("in_flight", 4)] + body)
    _same(got, _single(fs, cam, [("size", w, h)] + body), "4 in flight, 640x360")


def test_size_change_mid_run(cornell):
    fs, cam = cornell
    script = [("size", 64, 48), ("svgf", 0, {}), ("svgf", 1, {}), ("size", 100, 52), ("svgf", 2, {}), ("cam", 1), ("svgf", 3, {}),
              ("buf", "primary_position")]
    got, _ = _multi([0, 0, 0], fs, cam, script)
    _same(got, _single(fs, cam, script), "64x48 -> 100x52")


def test_reset_mid_run(cornell):
    fs, cam = cornell
    script = [("size", 64, 48), ("svgf", 0, {}), ("cam", 1), ("svgf", 1, {}), ("reset",), ("svgf", 0, {}), ("cam", 2), ("svgf", 1, {}),
              ("buf", "prev_moment_temporalweight")]
    got, _ = _multi([0, 0, 0], fs, cam, script)
    _same(got, _single(fs, cam, script), "reset")


def test_mixed_with_the_plain_renderer(cornell):
    """atn_mgpu_render, atn_mgpu_svgf_render, atn_mgpu_render on one handle, as the same mix on one context."""
    fs, cam = cornell
    script = [("size", 100, 52), ("render", 0), ("svgf", 0, {}), ("render", 1), ("cam", 1), ("svgf", 1, {}), ("render", 2)]
    got, _ = _multi([0, 0, 0], fs, cam, script)
    _same(got, _single(fs, cam, script), "mix")


def test_exchange_kernels_are_timed_where_they_run(cornell):
    """destination.profile = 1: one pack launch per frame on every shard but the first, one unpack launch per frame on the first --
    shard 0 neither packs nor pushes -- and a profiled frame is the same frame."""
    from aten_amd.renderer import MultiGpuPathTracing
    fs, cam = cornell
    w, h = 100, 52
    want = _single(fs, cam, [("size", w, h), ("svgf", 0, dict(stages=False)), ("svgf", 1, dict(stages=False))])
    m = MultiGpuPathTracing([0, 0, 0])
    try:
        got = _play(m, fs, cam, [("size", w, h), ("svgf", 0, dict(stages=False, profile=True)), ("svgf", 1, dict(stages=False, profile=True))])
        times = [m.kernel_times(i) for i in range(3)]
        assert [t["svgf_pack"][1] for t in times] == [0, 2, 2]
        assert [t["svgf_unpack"][1] for t in times] == [2, 0, 0]
        assert all(t["svgf_prepare"][1] == 0 for t in times[1:]) and times[0]["svgf_prepare"][1] > 0        # the filters ran on shard 0 only
        assert all(t["shade"][1] > 0 for t in times)                                                         # the path pass on every shard
        m.reset_kernel_times()
        assert all(n == 0 for i in range(3) for _, n in m.kernel_times(i).values())
    finally:
        m.close()
    _same(got, want, "profiled frames")


def test_refusals(cornell):
    from aten_amd._lib import lib
    from aten_amd.renderer import AtenAmdError, MultiGpuPathTracing, PathTracing
    fs, cam = cornell
    w, h = 16, 16
    m = MultiGpuPathTracing([0, 0])
    try:
        m.UpdateSceneData(fs)
        m.updateCamera(create_camera(cam["pos"], cam["at"], cam["vfov"], w, h))
        m.initSampler(w, h, 0)
        with pytest.raises(AtenAmdError, match=r"geometry history.*\(status -5\)"):        # ATN_ERR_UNSUPPORTED, and why
            m.svgf_render(w, h, compute_motion=2)
        with pytest.raises(AtenAmdError, match=r"motion/depth.*\(status -1\)"):             # ATN_ERR_INVALID_ARG
            m.svgf_render(w, h, compute_motion=0)
        img = m.svgf_render(w, h, compute_motion=True)          # neither refusal moved a shard: the handle still renders frame 0
        assert np.isfinite(img[..., :3]).all()
    finally:
        m.close()
    l = lib()
    assert l.atn_mgpu_svgf_render(None, None, 1, None, None) == -1
    assert l.atn_mgpu_svgf_set_motion_depth(None, None, 0) == -1
    assert l.atn_mgpu_svgf_reset(None) == -1
    assert l.atn_mgpu_svgf_set_atrous_iterations(None, 5) == -1
    assert l.atn_mgpu_svgf_set_dilate_temporal_weight(None, 0) == -1
    assert l.atn_mgpu_svgf_download(None, 13, None) == -1
    assert l.atn_mgpu_svgf_output_device(None) is None
    # a single context with a screen shard keeps refusing: the node-wide path does not go through atn_svgf_render
    r = PathTracing(0)
    try:
        r.UpdateSceneData(fs)
        r.updateCamera(create_camera(cam["pos"], cam["at"], cam["vfov"], w, h))
        r.initSampler(w, h, 0)
        r.setScreenShard(0, 2)
        with pytest.raises(AtenAmdError, match="one GPU"):
            r.svgf_render(w, h, compute_motion=True)
    finally:
        r.close()


def test_every_visible_gpu(cornell):
    import torch
    fs, cam = cornell
    script = [("size", 100, 52), ("svgf", 0, {}), ("cam", 1), ("svgf", 1, {}), ("svgf", 2, {})]
    got, n = _multi(None, fs, cam, script)
    assert n == torch.cuda.device_count() >= 1
    _same(got, _single(fs, cam, script), "devices=None")
