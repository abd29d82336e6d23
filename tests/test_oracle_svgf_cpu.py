"""CPU tests of the SVGF restatement (oracle/orc_svgf.h): self-consistency and the committed vectors."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import GOLDEN, make_camera


def _golden_module():
    spec = importlib.util.spec_from_file_location("make_golden_svgf", os.path.join(GOLDEN, "make_golden_svgf.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_aov_packing_known_answers_from_reference_unittest(orc):
    """src/aten_unittest/aov_host_buffer.cpp:73-108 `FillBasicAOVsTest` and :110-132 `FillBasicAOVsIfHitMissTest`, restated:
    normal (1,2,3), rec.p = vec4(1), identity mtx_W2C, albedo (4,5,6,7), isect.meshid = 2
      -> normal_depth == (normal.xyz, rec.p.z), albedo_meshid == (albedo.xyz, meshid)      (ASSERT_EQ: exact)
    bg (4,5,6,7) -> normal_depth == (0,0,0,-1), albedo_meshid == (bg.xyz, -1).
    The reference's own known answer for the SVGF AOV packing; the GPU planes are held to the same numbers
    in tests/test_gpu_invariants.py::test_svgf_aov_planes_known_answers."""
    normal, p, albedo = (1.0, 2.0, 3.0), (1.0, 1.0, 1.0), (4.0, 5.0, 6.0, 7.0)
    nd, am = orc.fill_basic_aovs(normal, p, np.eye(4, dtype=np.float32), albedo, 2)
    assert nd.tolist() == [1.0, 2.0, 3.0, 1.0]          # .w == rec.p.z (== clip w of (1,1,1,1) under identity)
    assert am.tolist() == [4.0, 5.0, 6.0, 2.0]
    # beyond the unit test's identity: depth is the CLIP-space w, i.e. row 3 of W2C applied to (p, 1) (aov.h:166-168)
    m = np.arange(16, dtype=np.float32).reshape(4, 4)
    nd, _ = orc.fill_basic_aovs(normal, (2.0, 3.0, 5.0), m, albedo, 2)
    assert nd[3] == np.float32(12 * 2 + 13 * 3 + 14 * 5 + 15)
    nd, am = orc.fill_basic_aovs_if_hit_miss((4.0, 5.0, 6.0, 7.0))
    assert nd.tolist() == [0.0, 0.0, 0.0, -1.0]
    assert am.tolist() == [4.0, 5.0, 6.0, -1.0]


def test_svgf_oracle_matches_committed_vectors():
    want = np.load(os.path.join(GOLDEN, "svgf_golden.npz"))
    got = _golden_module().run()
    assert set(got) == set(want.files)
    for k in want.files:
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), k


def test_svgf_oracle_behaviour(orc, cornell):
    fs, cam = cornell
    w, h = 64, 40
    c = make_camera(orc, cam, w, h)
    seeds = orc.init_sampler(w, h, 0)
    sv = orc.Svgf()
    try:
        films = []
        for frame in range(5):
            film, st = sv.render(fs, c, seeds, w, h, 3, 3, frame=frame, compute_motion=True, stages=True)
            films.append(film)
            md = sv.buffer("motion_depth")
            hit = sv.buffer("primary_position")[..., 3] == 1.0
            if frame > 0:
                assert np.all(md[..., :2] == 0.0)              # static camera: prev and cur NDC are the same floats
            # AOV depth = clip w = distance along the view direction (float64 check)
            p = sv.buffer("primary_position")[..., :3].astype(np.float64)
            d = np.asarray(cam["at"], np.float64) - np.asarray(cam["pos"], np.float64)
            d /= np.linalg.norm(d)
            depth = (p - np.asarray(cam["pos"], np.float64)) @ d
            nd = sv.buffer("prev_normal_depth")
            # (pixels that see the Specular box carry the AOV of the reflected hit, svgf.cpp:142-157)
            close = np.isclose(nd[..., 3][hit], depth[hit], rtol=1e-5, atol=1e-5)
            assert close.mean() > 0.9
            assert np.all(nd[..., 3][~hit] == -1.0)
            mt = sv.buffer("prev_moment_temporalweight")
            assert mt[..., 2].max() == frame + 1                # accumulated frame count of undisturbed pixels
            assert mt[..., 2].min() >= 1
        # the filtered frame is smoother than the path-traced one: mean absolute Laplacian drops
        def rough(a):
            a = np.nan_to_num(a[..., :3])
            return np.abs(4 * a[1:-1, 1:-1] - a[:-2, 1:-1] - a[2:, 1:-1] - a[1:-1, :-2] - a[1:-1, 2:]).mean()
        albedo = sv.buffer("prev_albedo_meshid")
        assert rough(films[-1]) < 0.7 * rough(st[0] * np.concatenate([albedo[..., :3], np.ones_like(albedo[..., :1])], -1))
    finally:
        sv.close()


def test_svgf_oracle_thread_count_independent(orc, cornell):
    fs, cam = cornell
    w, h = 48, 32
    c = make_camera(orc, cam, w, h)
    seeds = orc.init_sampler(w, h, 0)
    outs = []
    for nt in (1, 4):
        sv = orc.Svgf()
        frames = [sv.render(fs, c, seeds, w, h, 3, 3, frame=f, compute_motion=True, nthreads=nt) for f in range(3)]
        sv.close()
        outs.append(np.stack(frames))
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))


ALL_BUFFERS = ("normal_depth", "albedo_meshid", "color_variance", "moment_temporalweight", "prev_normal_depth", "prev_albedo_meshid",
               "prev_color_variance", "prev_moment_temporalweight", "temporary_color", "motion_depth", "primary_position", "atrous0", "atrous1")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("size", [(37, 21), (64, 40)])
def test_svgf_denoise_on_render_planes_equals_render(orc, cornell, size):
    """Svgf.denoise is the filter half of Svgf.render on a caller's planes: fed, frame after frame, the contributions and the
    G-buffer that render's path pass produced, it leaves the same film, the same stages and the same thirteen buffers, to the bit.
    (With tests/golden/svgf_golden.npz unchanged, this pins the split of orc_svgf_render into path pass + svgf_filter_passes.)"""
    fs, cam = cornell
    w, h = size
    c = make_camera(orc, cam, w, h)
    seeds = orc.init_sampler(w, h, 0)
    a, b = orc.Svgf(), orc.Svgf()
    try:
        for frame in range(3):
            want, wst = a.render(fs, c, seeds, w, h, 3, 3, frame=frame, compute_motion=True, stages=True)
            contribs = wst[0].copy()
            contribs[..., 3] = 1.0          # Path.contrib.samples with 1 spp
            got, gst = b.denoise(c, contribs, a.buffer("prev_normal_depth"), a.buffer("prev_albedo_meshid"), a.buffer("primary_position"),
                                 frame=frame, compute_motion=True, stages=True)
            assert np.array_equal(_bits(got), _bits(want)), frame
            assert np.array_equal(_bits(gst), _bits(wst)), frame
            for name in ALL_BUFFERS:
                assert np.array_equal(_bits(b.buffer(name)), _bits(a.buffer(name))), (frame, name)
        assert np.nanmax(want[..., :3]) > 0
    finally:
        a.close(); b.close()


def test_svgf_set_buffer_round_trips(orc):
    """set_buffer is the inverse of buffer: every plane comes back as it was set, the other planes keep their initial texels, and
    current / previous address the two AOV sets."""
    w, h = 5, 3
    rng = np.random.default_rng(7)
    sv = orc.Svgf()
    try:
        data = {name: rng.standard_normal((h, w, 4)).astype(np.float32) for name in ALL_BUFFERS}
        sv.set_buffer("atrous0", data["atrous0"])
        assert np.array_equal(_bits(sv.buffer("atrous0")), _bits(data["atrous0"]))
        init = np.tile(np.array([0, 0, 0, 1], np.float32), (h, w, 1))
        for name in ("normal_depth", "prev_moment_temporalweight", "atrous1", "temporary_color"):
            assert np.array_equal(sv.buffer(name), init), name
        for name in ALL_BUFFERS:
            sv.set_buffer(name, data[name])
        for name in ALL_BUFFERS:
            assert np.array_equal(_bits(sv.buffer(name)), _bits(data[name])), name
        with pytest.raises(ValueError):
            sv.set_buffer("atrous0", np.zeros((h + 1, w, 4), np.float32))      # another size than the renderer's buffers
    finally:
        sv.close()


def test_svgf_planes_generator_is_what_it_says():
    """tests/svgf_planes.py: deterministic, finite, and on the edges -- background singly, on the top row, on the right column and
    in a corner; every variance branch (frame counts 1 / 2-3 / >= 4) in the history; motion that leaves the frame on all four sides;
    one region of depth exactly 0 in the current planes and none in the history."""
    import svgf_planes as sp
    for w, h in sp.SIZES:
        for frame in sp.FRAMES:
            pl, hist = sp.planes(w, h, frame), sp.history(w, h, frame)
            again = sp.planes(w, h, frame)
            for k, v in list(pl.items()) + list(hist.items()):
                assert v.shape == (h, w, 4) and v.dtype == np.float32 and np.all(np.isfinite(v)), (w, h, frame, k)
            assert all(np.array_equal(pl[k], again[k]) for k in pl)
            assert pl["contribs"][..., :3].min() >= 0 and pl["contribs"][..., :3].max() <= 2 and np.all(pl["contribs"][..., 3] == 1)
            assert np.all(hist["prev_normal_depth"][..., 3] != 0)
            assert set(np.unique(hist["prev_moment_temporalweight"][..., 2])) <= {1.0, 2.0, 3.0, 4.0, 7.0}
    w, h = 67, 33
    pl, hist = sp.planes(w, h, 1), sp.history(w, h, 1)
    bg = pl["albedo_meshid"][..., 3] < 0
    assert bg[h - 1].sum() >= 2 and bg[:, w - 1].sum() >= 2 and bg[0, 0] and bg[1:-1, 1:-1].any()
    assert np.all(pl["normal_depth"][bg] == (0, 0, 0, -1))
    ids = pl["albedo_meshid"][..., 3]
    assert len(np.unique(ids[~bg])) == 6
    for edge in (ids[0], ids[-1], ids[:, 0], ids[:, -1]):
        assert (edge >= 0).any()
    assert (pl["normal_depth"][..., 3] == 0).any()
    px, py = pl["motion_depth"][..., 0] * w, pl["motion_depth"][..., 1] * h
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    assert (x + px < 0).any() and (x + px >= w).any() and (y + py < 0).any() and (y + py >= h).any()
    assert (px == 0).any() and ((px != 0) & (np.abs(px) < 1)).any() and np.isclose(px, 4.0).any()      # zero, sub-pixel, whole-pixel
    counts = hist["prev_moment_temporalweight"][..., 2]
    for edge in (counts[0], counts[-1], counts[:, 0], counts[:, -1]):
        assert {1.0, 2.0, 4.0} <= set(edge.tolist())


CONDITIONING_CAP = 2.5e-4       # a quarter of the frame tolerance 1e-3


def test_svgf_oracle_is_well_conditioned_on_the_synthetic_planes(orc, cornell):
    """The every-pixel comparisons of tests/test_gpu_svgf_edges.py hold the GPU to |gpu - cpu| <= 1e-3 * max(1, |cpu|) at EVERY pixel.
    That is fair only if the reference itself does not move by that much when its inputs move by what the kernels' documented
    substitutions amount to (pow128 by squarings, __expf, reciprocal-then-multiply: up to ~2^-18 relative).  So: every size and
    frame of svgf_planes, every a-trous level (iteration counts 1..5: the plane the last level wrote), once on the generated planes
    and once with every float of the colours, the history's colours and moments and the depths moved by a random relative amount
    of up to 2^-18 (ids, normals and frame counts stay) -- the two runs may differ by at most 2.5e-4 * max(1, |ref|), a quarter of
    the tolerance, at every pixel of the variance stage, of every level, of temporary_color and of the output.
    Measured worst value over all sizes, frames and levels: 1.86e-5 (67 x 33, frame 2, one level, output) -- a thirteenth of the
    cap; the test prints it."""
    import svgf_planes as sp
    _, cam = cornell
    worst = (0.0, None)
    for w, h in sp.SIZES:
        c = make_camera(orc, cam, w, h)
        for frame in sp.FRAMES:
            pl, hist = sp.planes(w, h, frame), sp.history(w, h, frame)
            rng = np.random.default_rng([w, h, frame, 99])
            pl2, hist2 = sp.perturbed(pl, rng, sp.PERTURB_PLANES), sp.perturbed(hist, rng, sp.PERTURB_HISTORY)
            for iters in (1, 2, 3, 4, 5):
                _, ref = sp.oracle_frame(orc, c, frame, pl, hist, iters=iters)
                _, mov = sp.oracle_frame(orc, c, frame, pl2, hist2, iters=iters)
                level = sp.last_level_plane(iters)
                for name, a, b in (("variance", mov["stages"][2], ref["stages"][2]), (level, mov[level], ref[level]),
                                   ("temporary_color", mov["temporary_color"][..., :3], ref["temporary_color"][..., :3]),
                                   ("output", mov["film"], ref["film"])):
                    assert np.all(np.isfinite(b)), (w, h, frame, iters, name)
                    rel = np.abs(a.astype(np.float64) - b) / np.maximum(1.0, np.abs(b))
                    if rel.max() > worst[0]:
                        worst = (float(rel.max()), (w, h, frame, iters, name))
                    assert rel.max() <= CONDITIONING_CAP, (w, h, frame, iters, name, float(rel.max()))
    print("conditioning: worst relative move %.3g at %s" % worst)
    assert worst[0] > 0        # the perturbation reached the outputs
