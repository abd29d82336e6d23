"""The SVGF filter passes at ragged and tiny frame sizes, EVERY pixel, against oracle/orc_svgf.h.

The sizes (svgf_planes.SIZES) are the smallest frames at which the kernels' index arithmetic takes each of its paths:
  1 x 1     every tap of every pass clamps to the one pixel
  5 x 3     smaller than every window (3 x 3, 5 x 5, 7 x 7, the +-32-pixel a-trous footprint)
  37 x 21   the width is no multiple of the 8-pixel tile of svgf_pixel, neither dimension a multiple of 2 * 2^i at any level i
  67 x 33   one pixel row in the second 32-row block, three columns in the ninth tile, gridDim.x rounded from 9 to 16 (seven
            tiles of every block row lie wholly outside the frame)
  130 x 1   one row          1 x 70   one column
The planes are synthetic (tests/svgf_planes.py): region edges, background pixels, motion that leaves the frame and every branch of
the variance pass sit on the frame edges.  Every frame starts from the SAME state on both sides -- the oracle's history and stale
current planes are uploaded into a context that was reset -- so frames 0..3 are compared on equal inputs and nothing accumulates.
The scene and camera are there only because atn_svgf_denoise wants a ready context.

Both a-trous kernels run: k_svgf_atrous4 (default) and k_svgf_atrous (ATEN_AMD_SVGF_ATROUS4=0).
"""
import os

import numpy as np
import pytest

import svgf_planes as sp
from conftest import make_camera, parity_record

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
INPUTS = ("contribs", "normal_depth", "albedo_meshid", "primary_position", "motion_depth")
KERNELS = {"0": "k_svgf_atrous", "1": "k_svgf_atrous4"}
TOL = 1e-3          # |gpu - cpu| <= TOL * max(1, |cpu|) per channel, DESIGN.md section 4 -- here at every pixel


@pytest.fixture(scope="module")
def contexts(cornell):
    """One context per a-trous kernel; ATEN_AMD_SVGF_ATROUS4 is read when a context is created."""
    from aten_amd.renderer import PathTracing
    fs, _ = cornell
    ctx = {}
    old = os.environ.get("ATEN_AMD_SVGF_ATROUS4")
    try:
        for flag in KERNELS:
            os.environ["ATEN_AMD_SVGF_ATROUS4"] = flag
            r = PathTracing(0)
            ctx[flag] = r
            r.UpdateSceneData(fs)
            r.setScreenShard(0, 1)
    finally:
        if old is None:
            os.environ.pop("ATEN_AMD_SVGF_ATROUS4", None)
        else:
            os.environ["ATEN_AMD_SVGF_ATROUS4"] = old
    yield ctx
    for r in ctx.values():
        r.close()


@pytest.fixture(scope="module")
def reference(orc, cornell):
    """The oracle's frames, computed once per (size, frame, iterations, dilation) and shared by the tests; never modified."""
    _, cam = cornell
    cache = {}

    def get(w, h, frame, iters=5, dilate=False):
        key = (w, h, frame, iters, dilate)
        if key not in cache:
            pl, hist = sp.planes(w, h, frame), sp.history(w, h, frame)
            before, after = sp.oracle_frame(orc, make_camera(orc, cam, w, h), frame, pl, hist, iters=iters, dilate=dilate)
            for d in (pl, before, after):
                for v in d.values():
                    v.setflags(write=False)
            cache[key] = (pl, before, after)
        return cache[key]
    return get


def _prepare(r, orc, cam, w, h):
    r.updateCamera(make_camera(orc, cam, w, h))
    r.initSampler(w, h, 0)


def gpu_frame(r, w, h, frame, pl, before, iters=5, dilate=False):
    """One frame of atn_svgf_denoise from exactly the oracle's state: a reset context (its buffers are re-initialised by the first
    upload, so frame 0 runs PrepareForDenoise on fresh texels), the input planes, the oracle's history and stale current planes,
    and a sentinel in every plane that only the passes write."""
    r.svgf_reset()
    r.svgf_set_atrous_iterations(iters)
    r.svgf_set_dilate_temporal_weight(dilate)
    for name in INPUTS:
        r.svgf_upload(name, pl[name])
    for name, v in before.items():
        r.svgf_upload(name, v)
    mark = np.full((h, w, 4), SENTINEL, np.float32)
    for name in ("output", "atrous0", "atrous1", "temporary_color"):
        r.svgf_upload(name, mark)
    film, st = r.svgf_denoise(w, h, frame=frame, compute_motion=False, stages=True)
    after = {name: r.svgf_buffer(name) for name in sp.HISTORY_PLANES + ("temporary_color", "atrous0", "atrous1", "output")}
    after["film"], after["stages"] = film, st
    return after


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("iters", [1, 5])
@pytest.mark.parametrize("flag", sorted(KERNELS))
@pytest.mark.parametrize("size", sp.SIZES, ids=lambda s: "%dx%d" % s)
def test_every_pixel_is_written(contexts, reference, orc, cornell, size, flag, iters):
    """A sentinel uploaded into `output`, both a-trous ping-pong planes and temporary_color before the call is gone afterwards from
    the output, from every plane an a-trous level wrote (with one level: the plane of level 0 only) and from temporary_color.xyz.
    Exact: a pixel that the block map, the group rounding or the valid / done handling leaves out keeps the sentinel."""
    w, h = size
    r = contexts[flag]
    _prepare(r, orc, cornell[1], w, h)
    try:
        for frame in sp.FRAMES:
            pl, before, _ = reference(w, h, frame, iters)
            got = gpu_frame(r, w, h, frame, pl, before, iters)
            written = ["output", "film", "temporary_color", sp.last_level_plane(iters)] + (["atrous0", "atrous1"] if iters > 1 else [])
            for name in written:
                left = np.argwhere(np.any(got[name] == SENTINEL, axis=-1))
                assert len(left) == 0, (KERNELS[flag], frame, name, "(y, x) never written:", left[:8].tolist())
            if iters == 1:      # ... and the plane no level writes is untouched
                assert np.all(got["atrous0"] == SENTINEL), (KERNELS[flag], frame)
            assert np.array_equal(_bits(got["output"]), _bits(got["film"]))
    finally:
        r.svgf_set_atrous_iterations(5)


@pytest.mark.parametrize("dilate", [False, True])
@pytest.mark.parametrize("size", sp.SIZES, ids=lambda s: "%dx%d" % s)
def test_exact_passes_at_the_edges(contexts, reference, orc, cornell, size, dilate):
    """No transcendental in temporal reprojection, moment accumulation, the optional 3 x 3 weight dilation and the background rule
    of the variance pass: with the external motion plane (vectors that leave the frame on every side) the temporal stage and the
    moment / temporal-weight plane agree with the oracle to the last bit at every size; the variance stage of a background pixel
    is exactly 0 and its moments are exactly (0, 0, 1, w)."""
    w, h = size
    r = contexts["1"]
    _prepare(r, orc, cornell[1], w, h)
    try:
        for frame in sp.FRAMES:
            pl, before, want = reference(w, h, frame, 5, dilate)
            got = gpu_frame(r, w, h, frame, pl, before, 5, dilate)
            assert np.array_equal(_bits(got["stages"][0]), _bits(want["stages"][0])), frame
            bad = np.argwhere(np.any(_bits(got["stages"][1]) != _bits(want["stages"][1]), axis=-1))
            assert len(bad) == 0, (frame, "temporal stage, (y, x):", bad[:8].tolist())
            a, b = got["prev_moment_temporalweight"], want["prev_moment_temporalweight"]
            bad = np.argwhere(np.any(_bits(a) != _bits(b), axis=-1))
            assert len(bad) == 0, (frame, "moments / temporal weight, (y, x):", bad[:8].tolist())
            for name in ("prev_normal_depth", "prev_albedo_meshid"):
                assert np.array_equal(_bits(got[name]), _bits(pl[name[5:]])), (frame, name)
            bg = pl["albedo_meshid"][..., 3] < 0
            assert np.all(got["stages"][2][bg] == 0.0), frame
            assert np.all(a[bg][:, :3] == (0.0, 0.0, 1.0)), frame
    finally:
        r.svgf_set_dilate_temporal_weight(False)


@pytest.mark.parametrize("flag", sorted(KERNELS))
@pytest.mark.parametrize("size", sp.SIZES, ids=lambda s: "%dx%d" % s)
def test_every_pixel_of_the_toleranced_passes(contexts, reference, orc, cornell, size, flag):
    """The variance stage, temporary_color (level 0), the ping-pong planes as every level count 1..5 leaves them (so the plane of
    EVERY level is compared as its last writer left it), the new colour / variance history and the output: inside
    |gpu - cpu| <= 1e-3 * max(1, |cpu|) at EVERY pixel and channel, no share left out.  Fair because the oracle itself moves by at
    most 1.9e-5 on these planes when its inputs move by the kernels' substitutions
    (tests/test_oracle_svgf_cpu.py::test_svgf_oracle_is_well_conditioned_on_the_synthetic_planes).  The worst per-pixel difference
    per size and kernel goes into the parity report."""
    w, h = size
    r = contexts[flag]
    _prepare(r, orc, cornell[1], w, h)
    worst = {}
    films = ([], [])
    try:
        for frame in sp.FRAMES:
            for iters in (1, 2, 3, 4, 5):
                pl, before, want = reference(w, h, frame, iters)
                got = gpu_frame(r, w, h, frame, pl, before, iters)
                planes = [("variance stage", got["stages"][2], want["stages"][2]),
                          ("temporary_color", got["temporary_color"], want["temporary_color"]),
                          ("prev_color_variance", got["prev_color_variance"], want["prev_color_variance"]),
                          ("level %d (%s)" % (iters - 1, sp.last_level_plane(iters)), got[sp.last_level_plane(iters)], want[sp.last_level_plane(iters)]),
                          ("output", got["film"], want["film"])]
                if iters > 1:
                    other = sp.last_level_plane(iters - 1)
                    planes.append(("level %d (%s)" % (iters - 2, other), got[other], want[other]))
                for name, a, b in planes:
                    assert np.all(np.isfinite(b)), (frame, iters, name)
                    rel = np.abs(a.astype(np.float64) - b) / np.maximum(1.0, np.abs(b))
                    rel = np.where(np.isfinite(rel), rel, np.inf)
                    key = name.split(" (")[0]
                    worst[key] = max(worst.get(key, 0.0), float(rel.max()))
                    print("%s %dx%d frame %d levels %d %-24s worst %.3g" % (KERNELS[flag], w, h, frame, iters, name, rel.max()))
                    bad = np.argwhere(np.any(rel > TOL, axis=-1))
                    assert len(bad) == 0, (KERNELS[flag], frame, iters, name, float(rel.max()), "(y, x):", bad[:8].tolist())
                if iters == 5:
                    films[0].append(got["film"]); films[1].append(want["film"])
    finally:
        r.svgf_set_atrous_iterations(5)
    parity_record("SVGF edges: synthetic planes %dx%d, %s, frames 0-3, filtered output of every pixel" % (w, h, KERNELS[flag]),
                  np.stack(films[0]), np.stack(films[1]), tol=TOL, worst_rel_err_per_plane=worst)
