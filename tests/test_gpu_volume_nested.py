"""Nested media, deep iterations and all three walks of the volume renderer on the GPU against the CPU twin
(tests/cxx/volume_oracle.cpp).  tests/volume_scenes.py has the scenes and the handle: a pixel that has only PASSED medium boundaries
up to iteration k has bit-equal inputs there on both sides, and makes its first decision with up to k media on its stack.
tests/test_volume_nested_cpu.py pins the sets (events at every depth, full and overflowing stacks, the walk bound, NO near tie in
any case used here), so nothing below is left out of a comparison and nothing passes by being empty.

Every stage test runs under the walk the context picks (the LDS copy of the node image), under ATEN_AMD_TRACE=r (the lane-refilling
walk: k_vol_closest<true, false>, k_vol_transmit<true, false>, a connection's next segment handed back to its lane) and under
ATEN_AMD_LDS_NODES=0 (the plain walk over global memory).  Both variables are read when the context is created.  A scene whose node
image cannot fit the 32 KB of the LDS copy runs under the two global walks only (volume_scenes.walks_for): the context's own choice
is then the plain global walk.  slab_row(33) is 26 .. 39 KB by the record sizes, so it keeps the third case, whichever walk that is.

Frames are 64 x 48 and a ragged 37 x 21, two frames each, sample 0, one capture per iteration 0 .. 7."""
import numpy as np
import pytest

from conftest import parity_record, ulp_diff

import volume_scenes as VS

pytestmark = pytest.mark.gpu

WALKS = ("own", "refill", "global")
FLAGS = ("processed", "hit", "sampled", "absorbed", "scattered", "passed", "connection", "terminated")


@pytest.fixture(scope="module")
def vq():
    import volume_oracle
    volume_oracle.lib()
    return volume_oracle


def _ctx(monkeypatch, walk, scene, cam, w, h):
    from aten_amd.renderer import PathTracing
    if walk == "refill":
        monkeypatch.setenv("ATEN_AMD_TRACE", "r")
    else:
        monkeypatch.delenv("ATEN_AMD_TRACE", raising=False)
    if walk == "global":
        monkeypatch.setenv("ATEN_AMD_LDS_NODES", "0")
    else:
        monkeypatch.delenv("ATEN_AMD_LDS_NODES", raising=False)
    r = PathTracing(0)
    try:
        r.UpdateSceneData(scene)
        r.updateCamera(cam)
        r.initSampler(w, h, 0)
    except Exception:
        r.close()
        raise
    return r


def _capture(r, w, h, frame, k, **kw):
    r.volume_reset()
    r.volume_capture(k)
    r.volume_render(w, h, frame=frame, **kw)
    return dict(state=r.volume_buffer("state"), ray=r.volume_buffer("ray"), conn=r.volume_buffer("conn"), stack=r.volume_buffer("stack"),
                counters=r.volume_buffer("counters"))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _cases(orc, vq, name, n, **kw):
    for w, h in VS.SIZES:
        for frame in VS.FRAMES:
            yield w, h, frame, VS.case(orc, vq, name, n, w, h, frame, **kw)


def _skip_walk(c, walk):
    return walk not in VS.walks_for(c["scene"])


# ---- 1. pass-only pixels: everything byte-equal, at every iteration and stack depth up to the full stack ---------------------------------
@pytest.mark.parametrize("walk", WALKS)
@pytest.mark.parametrize("n", (8, 12))
def test_pass_only_pixels_are_byte_equal(monkeypatch, orc, vq, n, walk):
    """`thin`: no events, every boundary is a pass, no mask beyond "still pass-only".  On every first-decision pixel (bit-equal
    inputs): the flags, the hit distance's bytes, s within 2 ulp.  On every pixel that passes at this iteration too: depth_count,
    stack size, the CMJ dimension, the eight stack entries and the next ray's origin and direction, byte for byte.  Both fill the
    stack at iteration 7 (eight ids across all four dwords); with n = 12 there are shells left to enter behind it."""
    seen_full = False
    for w, h, frame, c in _cases(orc, vq, "thin", n):
        r = _ctx(monkeypatch, walk, c["scene"], c["cam"], w, h)
        try:
            worst = 0
            for k in range(VS.ITERATIONS):
                g, t, m = _capture(r, w, h, frame, k), c["stages"][k], c["masks"][k]
                what = "thin n %d, %s walk, %d x %d frame %d iteration %d" % (n, walk, w, h, frame, k)
                assert m.sum() > 0, what
                for f in ("processed", "hit", "sampled", "absorbed", "scattered", "passed"):
                    assert np.array_equal(g["state"][f][m], t["state"][f][m]), (what, f)
                assert np.array_equal(_bits(g["ray"]["hit_t"][m]), _bits(t["ray"]["hit_t"][m])), what
                sd = int(ulp_diff(g["ray"]["s"][m], t["ray"]["s"][m]).max())
                worst = max(worst, sd)
                assert sd <= 2, (what, sd)
                po = m & VS.pass_only(t)
                assert po.sum() > 0, what
                for f in FLAGS:
                    assert np.array_equal(g["state"][f][po], t["state"][f][po]), (what, f)
                for f in ("depth_count", "stack_size", "dim"):
                    assert np.array_equal(g["state"][f][po], t["state"][f][po]), (what, f)
                assert np.array_equal(g["stack"][po], t["stack"][po]), what
                assert np.array_equal(_bits(g["ray"]["org"][po]), _bits(t["ray"]["org"][po])), what
                assert np.array_equal(_bits(g["ray"]["dir"][po]), _bits(t["ray"]["dir"][po])), what
                seen_full = seen_full or bool((g["state"]["stack_size"][po] == 8).any())
            print("thin n %d, %s walk, %d x %d frame %d: s max %d ulp over iterations 0 .. 7" % (n, walk, w, h, frame, worst))
        finally:
            r.close()
    assert seen_full


# ---- 2. the first decision with k media on the stack ----------------------------------------------------------------------------------
@pytest.mark.parametrize("walk", WALKS)
@pytest.mark.parametrize("name", ("outer_dense", "outer_thin"))
def test_first_decision_under_k_media(monkeypatch, orc, vq, name, walk):
    """Iterations 1 .. 7 on the first-decision mask, the assertions of test_gpu_volume.py::test_stage_parity unchanged: s within
    2 ulp, every flag, the CMJ dimension, depth_count, the stack and its size exact, scattered directions within 2e-5.  No pixel is
    left out for a near tie: there is none (tests/test_volume_nested_cpu.py).  outer_thin: the device makes the twin's events and
    no other -- a kernel that sampled the newest medium instead of the first would make hundreds."""
    for w, h, frame, c in _cases(orc, vq, name, 8):
        r = _ctx(monkeypatch, walk, c["scene"], c["cam"], w, h)
        try:
            events_gpu = events_twin = 0
            for k in range(1, VS.ITERATIONS):
                g, t, m = _capture(r, w, h, frame, k), c["stages"][k], c["masks"][k]
                what = "%s, %s walk, %d x %d frame %d iteration %d" % (name, walk, w, h, frame, k)
                gs, ts = g["state"], t["state"]
                assert m.sum() > 0, what
                assert VS.near_ties(t, m).sum() == 0, what
                assert np.array_equal(gs["processed"][m], ts["processed"][m]) and ts["processed"][m].all(), what
                assert np.array_equal(gs["sampled"][m], ts["sampled"][m]), what
                assert np.array_equal(_bits(g["ray"]["hit_t"][m]), _bits(t["ray"]["hit_t"][m])), what
                sd = ulp_diff(g["ray"]["s"][m], t["ray"]["s"][m])
                assert sd.max() <= 2, what
                for f in ("absorbed", "scattered", "passed", "connection", "terminated"):
                    assert np.array_equal(gs[f][m], ts[f][m]), (what, f)
                assert np.array_equal(gs["dim"][m], ts["dim"][m]), what
                assert np.array_equal(gs["depth_count"][m], ts["depth_count"][m]), what
                assert np.array_equal(gs["stack_size"][m], ts["stack_size"][m]), what
                assert np.array_equal(g["stack"][m], t["stack"][m]), what
                sc = m & ts["scattered"]
                dd = 0.0
                if sc.any():
                    dd = float(np.abs(g["ray"]["dir"][sc] - t["ray"]["dir"][sc]).max())
                    assert dd <= 2e-5, what
                print("%s: %d pixels, stack up to %d, s max %d ulp, %d scattered (direction max %.3g), %d absorbed"
                      % (what, m.sum(), ts["stack_size"][m].max(), sd.max(), sc.sum(), dd, (m & ts["absorbed"]).sum()))
                events_gpu += int((m & (gs["scattered"] | gs["absorbed"])).sum())
                events_twin += int((m & VS.events(t)).sum())
            assert events_gpu == events_twin
            if name == "outer_dense" and (w, h) == VS.SIZES[0]:
                assert events_twin >= 7 * 20
        finally:
            r.close()


# ---- 3. connections through nested boundaries --------------------------------------------------------------------------------------------
def _compare_connections(g, t, m, what):
    """Where the record is bit-equal: visible and segments exact, transmittance within 1e-5 relative -> (connections, bit-equal mask)."""
    gc, tc = g["conn"], t["conn"]
    conn = m & t["state"]["connection"]
    assert np.array_equal(g["state"]["connection"][m], t["state"]["connection"][m]), what
    same = conn & np.all(_bits(gc["org"]) == _bits(tc["org"]), -1) & np.all(_bits(gc["dir"]) == _bits(tc["dir"]), -1) \
        & (_bits(gc["t_max"]) == _bits(tc["t_max"]))
    assert np.array_equal(gc["visible"][same], tc["visible"][same]), what
    assert np.array_equal(gc["segments"][same], tc["segments"][same]), what
    if same.any():
        rel = np.abs(gc["transmittance"][same] - tc["transmittance"][same]) / np.maximum(np.abs(tc["transmittance"][same]), 1e-30)
        assert rel.max() <= 1e-5, (what, float(rel.max()))
    return conn, same


@pytest.mark.parametrize("walk", WALKS)
def test_connections_through_nested_boundaries(monkeypatch, orc, vq, walk):
    """outer_dense, iterations 0 .. 7, the first-decision pixels' connections: surface connections from exact floor hits through up
    to eight shell boundaries (the connection's own copy of the stack pushed and popped on the way), event connections from inside
    the shells.  Coverage is a condition: at iteration 0 of the 64 x 48 frames at least 200 bit-equal records walk 3 segments or
    more.  The measured bit-equal share goes to the parity report."""
    for w, h, frame, c in _cases(orc, vq, "outer_dense", 8):
        r = _ctx(monkeypatch, walk, c["scene"], c["cam"], w, h)
        try:
            shares, counts, got, want = [], [], [], []
            for k in range(VS.ITERATIONS):
                g, t, m = _capture(r, w, h, frame, k), c["stages"][k], c["masks"][k]
                what = "outer_dense, %s walk, %d x %d frame %d iteration %d" % (walk, w, h, frame, k)
                conn, same = _compare_connections(g, t, m, what)
                assert conn.sum() > 0 and same.sum() > 0, what
                if k == 0 and (w, h) == VS.SIZES[0]:
                    assert (same & (t["conn"]["segments"] >= 3)).sum() >= 200, what
                shares.append(float(same.sum()) / float(conn.sum()))
                counts.append(int(conn.sum()))
                got.append(g["conn"]["transmittance"][same]); want.append(t["conn"]["transmittance"][same])
                print("%s: %d connections, %d bit-equal records, up to %d segments" % (what, conn.sum(), same.sum(), t["conn"]["segments"][same].max()))
            got, want = np.concatenate(got), np.concatenate(want)
            parity_record("volume_nested_connections_outer_dense_%s_%dx%d_frame%d" % (walk, w, h, frame), got[:, None], want[:, None],
                          tol=1e-5, quantity="transmittance of the bit-equal connection records of the first-decision pixels",
                          connections_by_iteration=counts, bit_equal_share_by_iteration=shares)
        finally:
            r.close()


@pytest.mark.parametrize("walk", WALKS)
@pytest.mark.parametrize("m", (33, 32))
def test_connections_through_a_row_of_slabs(monkeypatch, orc, vq, m, walk):
    """Every pixel's connection from the wall crosses 2 m boundaries of a medium that attenuates, one medium on the stack at most:
    65 segments, visible with 32 slabs, blocked at the 65th boundary with 33; the product of 32 (33) factors within 1e-5 relative
    (each factor an expf of <= 2 ulp and a rounding: 33 x 4 x 6e-8 at the worst)."""
    for w, h, frame, c in _cases(orc, vq, "slab_row_dense", m):
        if _skip_walk(c, walk):
            continue
        r = _ctx(monkeypatch, walk, c["scene"], c["cam"], w, h)
        try:
            g, t = _capture(r, w, h, frame, 0), c["stages"][0]
            what = "slab_row(%d), %s walk, %d x %d frame %d" % (m, walk, w, h, frame)
            conn, same = _compare_connections(g, t, c["masks"][0], what)
            assert conn.all()
            print("%s: %d connections, %d bit-equal records" % (what, conn.sum(), same.sum()))
            assert same.sum() >= min(200, conn.sum() // 4), what       # coverage, as for the shells: 200 of the 64 x 48 frame's 3072
            assert np.all(t["conn"]["segments"][same] == 65) and np.all(t["conn"]["visible"][same] == (m == 32))
            assert g["counters"]["stack_overflow"] == 0
        finally:
            r.close()


# ---- 4. the frame's counters, exact ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("walk", WALKS)
@pytest.mark.parametrize("name,n", [("thin", 12), ("slab_row", 33), ("slab_row", 32)])
def test_counters_equal_the_twin(monkeypatch, orc, vq, name, n, walk):
    """max_depth 1, media without events: every connection starts on a first-decision pixel (confirmed on the twin), so dropped
    pushes, walks cut at the 64th boundary, connections and segments of the frame equal the twin's, number for number."""
    for w, h, frame, c in _cases(orc, vq, name, n, max_depth=VS.COUNTER_MAX_DEPTH):
        if _skip_walk(c, walk):
            continue
        r = _ctx(monkeypatch, walk, c["scene"], c["cam"], w, h)
        try:
            r.volume_reset()
            r.volume_render(w, h, frame=frame, max_depth=VS.COUNTER_MAX_DEPTH)
            got, want = r.volume_buffer("counters"), c["counters"]
            print("%s %d, %s walk, %d x %d frame %d: %r" % (name, n, walk, w, h, frame, got))
            assert got == want, (name, n, walk, w, h, frame)
            assert (got["stack_overflow"] > 0) == (name == "thin")
            assert (got["walk_overflow"] > 0) == ((name, n) == ("slab_row", 33))
            assert got["connections"] > 0 and got["segments"] > got["connections"]
        finally:
            r.close()


# ---- 5. the three walks give the same bytes -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ("cornell_box_smoke", "outer_dense"))
def test_films_are_byte_equal_across_the_walks(monkeypatch, orc, which):
    """128 x 96, 2 samples per pixel, four progressive frames under the LDS copy, the lane-refilling walk and the plain global walk:
    the same records, the same arithmetic, the same order of additions per path."""
    from aten_amd.scene import scenedefs
    w, h = 128, 96
    scene, cam = scenedefs.cornell_box_smoke() if which == "cornell_box_smoke" else VS.nested_shells(8, "outer_dense")[:2]
    c = orc.create_camera(cam["pos"], cam["at"], cam["vfov"], w, h)
    films = {}
    for walk in WALKS:
        r = _ctx(monkeypatch, walk, scene, c, w, h)
        try:
            films[walk] = [r.volume_render(w, h, spp=2, frame=f).copy() for f in range(4)]
        finally:
            r.close()
    assert all(np.isfinite(f).all() for f in films["own"]) and films["own"][3][..., :3].max() > 0
    for walk in WALKS[1:]:
        for f, (a, b) in enumerate(zip(films["own"], films[walk])):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (which, walk, f)


# ---- 6. the film of a nested scene ----------------------------------------------------------------------------------------------------------
_twin_films = {}


@pytest.mark.parametrize("walk", WALKS)
def test_nested_frame_parity(monkeypatch, orc, vq, walk):
    """Five progressive frames of outer_dense against the twin under the frame contract of test_gpu_volume.py::test_frame_parity:
    99.5 % of the pixels within 1e-3 max(1, |twin|), the image mean within 5e-3 relative."""
    w, h = 128, 96
    scene, cam, _ = VS.nested_shells(8, "outer_dense")
    c = orc.create_camera(cam["pos"], cam["at"], cam["vfov"], w, h)
    seeds = orc.init_sampler(w, h, 0)
    if not _twin_films:
        v = vq.Volume()
        for f in range(5):
            _twin_films[f] = v.render(scene, c, seeds, w, h, frame=f)
    r = _ctx(monkeypatch, walk, scene, c, w, h)
    try:
        worst = 100.0
        for f in range(5):
            got, want = r.volume_render(w, h, frame=f), _twin_films[f]
            m = parity_record("volume_nested_outer_dense_%s_frame%d" % (walk, f), got, want)
            inside = 100.0 * float(np.mean(np.all(np.abs(got - want) <= 1e-3 * np.maximum(1.0, np.abs(want)), axis=-1)))
            mean_rel = abs(float(got[..., :3].mean()) - float(want[..., :3].mean())) / max(float(want[..., :3].mean()), 1e-30)
            print("outer_dense %s walk frame %d: %.3f %% inside, image-mean rel %.3g" % (walk, f, inside, mean_rel), m)
            worst = min(worst, inside)
            assert mean_rel <= 5e-3
        cnt = r.volume_buffer("counters")
        assert cnt["stack_overflow"] == 0 and cnt["walk_overflow"] == 0
        assert worst >= 99.5
    finally:
        r.close()
