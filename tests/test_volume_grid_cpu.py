"""The CPU twin of the volume renderer with grid media (tests/cxx/volume_grid_oracle.cpp) on its own: it equals the old twin where no
grid is named, its tracking loops (the product's aten_amd/csrc/device/volume_grid_track.h) meet their closed forms and a flight
worked by hand, a grid of constant density is the homogeneous medium in expectation, and the scenes of tests/test_gpu_volume_grid.py
meet the gates those tests rest on.  docs/VOLUME.md, "Grid media"."""
import struct

import numpy as np
import pytest

import volume_grid_oracle as VG
import volume_oracle as V
from conftest import make_camera


def _scene(name, **kw):
    from aten_amd.scene import scenedefs
    return getattr(scenedefs, name)(**kw)


# ---- 1. no grid named: the old twin, byte for byte ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell_box_medium", "cornell_box_smoke", "cornell_box_subsurface"])
def test_old_and_new_twin_agree_without_grids(orc, name):
    """48 x 32, 2 progressive frames: the film and the state after every iteration."""
    w, h = 48, 32
    fs, cam = _scene(name)
    c = make_camera(orc, cam, w, h)
    seeds = orc.init_sampler(w, h, 0)
    for it in range(8):
        old, new = V.Volume(), VG.Volume()
        for f in range(2):
            fo, so = old.render(fs, c, seeds, w, h, frame=f, capture=it)
            fn, sn = new.render(fs, c, seeds, w, h, frame=f, capture=it)
            assert np.array_equal(fo.view(np.uint32), fn.view(np.uint32))
            for part in ("state", "ray", "conn"):
                for k, a in so[part].items():
                    assert np.array_equal(np.asarray(a).view(np.uint8), np.asarray(sn[part][k]).view(np.uint8)), (part, k, it, f)
            assert np.array_equal(so["stack"], sn["stack"])
            assert sn["conn"]["track_steps"].max() == 0 and sn["conn"]["stream_dim"].max() == 0 and sn["ties"].max() == 0
            assert {k: new.counters[k] for k in old.counters} == old.counters
            assert new.counters["flight_capped"] == 0 and new.counters["connection_capped"] == 0


# ---- 2. the tracking loops against closed forms -----------------------------------------------------------------------------------------
CONSTANT = (np.full((4, 4, 4), 0.8, np.float32), (0.0, 0.0, 0.0), 0.5)      # the box [0, 2]^3, density 0.8
ORG, DIR = (-1.0, 1.01, 0.97), (1.0, 0.0, 0.0)                              # enters the box at t = 1, leaves it at t = 3
SIGMA_S = 1.5
N = 65536


def _scrambles():
    return np.random.default_rng(5).integers(1, 2 ** 32, N, dtype=np.uint64).astype(np.uint32)


@pytest.mark.parametrize("length, chord", [(4.0, 2.0), (2.0, 1.0), (1.5, 0.5)])
def test_tracking_means_meet_their_closed_forms(length, chord):
    """A constant grid, majorant = EvalMajorant: over 65 536 streams the mean transmittance of ratio tracking is exp(-sigma * chord)
    and the event fraction of delta tracking 1 - exp(-sigma * chord), within 4 standard errors; a walk of length 2.0 or 1.5 ends
    inside the box.  Delta tracking also under a majorant 2.5 times too large (null collisions)."""
    majorant = float(np.float32(SIGMA_S) * np.float32(0.8))
    p = np.exp(-majorant * chord)
    se = np.sqrt(p * (1 - p) / N)
    scr = _scrambles()
    tr = VG.ratio_track(CONSTANT, SIGMA_S, majorant, ORG, DIR, length, scr)
    assert not tr["capped"].any()
    print("length %g: transmittance %.5f, closed form %.5f, %.2f standard errors" % (length, tr["tr"].mean(), p, (tr["tr"].mean() - p) / se))
    assert abs(tr["tr"].mean() - p) <= 4 * se
    for mj in (majorant, 2.5 * majorant):
        ev = VG.delta_track(CONSTANT, SIGMA_S, mj, ORG, DIR, length, scr)
        frac = (ev["kind"] == VG.KINDS["scatter"]).mean()
        assert set(np.unique(ev["kind"])) <= {VG.KINDS["end"], VG.KINDS["scatter"]}
        print("length %g majorant %.2f: events %.5f, closed form %.5f, %.2f standard errors, %.2f steps" % (length, mj, frac, 1 - p, (frac - (1 - p)) / se, ev["steps"].mean()))
        assert abs(frac - (1 - p)) <= 4 * se
        inside = ev["kind"] == VG.KINDS["scatter"]
        assert (ev["s"][inside] >= 1.0).all() and (ev["s"][inside] < min(length, 3.0)).all()
        assert (ev["s"][~inside] == np.float32(min(length, 3.0))).all()


def test_ratio_tracking_under_a_loose_majorant_is_the_reference_s_as_written():
    """medium.cpp:192-198 lets a collision both survive with probability sigma_n / majorant and weight the walk by it: with a
    majorant larger than sigma the mean is exp(-sigma * chord * (2 - sigma / majorant)), not exp(-sigma * chord).  Kept as written
    (docs/VOLUME.md, quirks); exact where majorant = sigma, which EvalMajorant gives a constant grid."""
    sigma = float(np.float32(SIGMA_S) * np.float32(0.8))
    mj = 2.0 * sigma
    tr = VG.ratio_track(CONSTANT, SIGMA_S, mj, ORG, DIR, 4.0, _scrambles())
    want = np.exp(-sigma * 2.0 * (2.0 - sigma / mj))
    se = tr["tr"].std() / np.sqrt(N)
    assert abs(tr["tr"].mean() - want) <= 4 * se
    assert abs(tr["tr"].mean() - np.exp(-sigma * 2.0)) > 4 * se


def test_a_ray_that_misses_the_box_draws_nothing():
    scr = _scrambles()[:256]
    ev = VG.delta_track(CONSTANT, SIGMA_S, 1.2, (-1.0, 2.5, 0.97), DIR, 10.0, scr)
    assert (ev["kind"] == VG.KINDS["miss"]).all() and (ev["draws"] == 2).all() and (ev["steps"] == 0).all()
    ev = VG.delta_track(CONSTANT, SIGMA_S, 1.2, ORG, DIR, 0.75, scr)       # the surface lies in front of the box
    assert (ev["kind"] == VG.KINDS["miss"]).all() and (ev["draws"] == 2).all()
    tr = VG.ratio_track(CONSTANT, SIGMA_S, 1.2, ORG, (-1.0, 0.0, 0.0), 10.0, scr)
    assert (tr["tr"] == 1.0).all() and (tr["steps"] == 0).all()


# ---- 3. a flight worked by hand ---------------------------------------------------------------------------------------------------------
def test_a_flight_by_hand():
    """A 2 x 1 x 1 grid, voxel 0 of density 1 and voxel 1 empty, box [0, 2] x [0, 1] x [0, 1]; the ray starts at x = -0.5 and runs along
    +x, so the clip is [0.5, 2.5]; sigma_s 1, majorant 2.  Stream (index 0, dimension 2, scramble 11) draws u, r per step:
      step 1: u 0.58186108  ds = -ln(1 - u) / 2 = 0.43597078  s 0.93597078  x 0.43597078  voxel 0, density 1: prob 0.5, r 0.54553396 -> null
      step 2: u 0.76735020  s 1.66508126  x 1.16508126  voxel 1, empty: prob 0 -> null
      step 3: u 0.07432944  s 1.70369971  x 1.20369971  voxel 1 -> null
      step 4: u 0.56121695  s 2.11557484  x 1.61557484  voxel 1 -> null
      step 5: u 0.82457006  s 2.98583269 >= 2.5: the flight ends at the box exit, 2.5, without an event; 9 draws."""
    grid = (np.array([[[1.0, 0.0]]], np.float32), (0.0, 0.0, 0.0), 1.0)
    o = VG.delta_track(grid, 1.0, 2.0, (-0.5, 0.5, 0.5), (1.0, 0.0, 0.0), 10.0, [11], log=8, dim=2)
    assert o["kind"][0] == VG.KINDS["end"] and o["steps"][0] == 5 and o["draws"][0] == 2 + 9 and o["s"][0] == np.float32(2.5)
    assert not o["tie"][0]
    u = o["log_draws"][0:10:2]
    r = o["log_draws"][1:8:2]
    assert np.allclose(u, [0.58186108, 0.76735020, 0.07432944, 0.56121695, 0.82457006], atol=5e-8, rtol=0)
    assert np.allclose(r, [0.54553396, 0.31182933, 0.86978889, 0.88690513], atol=5e-8, rtol=0)
    # by hand, in the loop's own precision: the logarithm in double, rounded once, the division and the sum in float
    s, want_s = np.float32(0.5), []
    for x in u:
        ds = np.float32(-np.float32(np.log(np.float64(np.float32(1.0) - x)))) / np.float32(2.0)
        s = np.float32(s + ds)
        want_s.append(s)
    assert np.array_equal(o["log_s"][:5], np.asarray(want_s, np.float32))
    assert np.allclose(want_s, [0.93597078, 1.66508126, 1.70369971, 2.11557484, 2.98583269], atol=2e-7, rtol=0)
    x = o["log_idx"][:4, 0]
    assert np.array_equal(x, (np.float32(-0.5) + np.asarray(want_s[:4], np.float32)).astype(np.float32))
    assert np.floor(x).astype(int).tolist() == [0, 1, 1, 1]
    assert r[0] >= 0.5                     # the one step that could have scattered did not
    # the same stream with voxel 0 twice as dense scatters at step 1: prob 1 > r
    dense = (np.array([[[2.0, 0.0]]], np.float32), (0.0, 0.0, 0.0), 1.0)
    o2 = VG.delta_track(dense, 1.0, 2.0, (-0.5, 0.5, 0.5), (1.0, 0.0, 0.0), 10.0, [11], log=8, dim=2)
    assert o2["kind"][0] == VG.KINDS["scatter"] and o2["steps"][0] == 1 and o2["s"][0] == want_s[0] and o2["draws"][0] == 4
    assert abs(o2["factor"][0] - 1.0) <= 2e-7      # tr * (sigma_s_at / prob_sigma_s) / (majorant * tr)
    # a surface at t = 1.7 ends the flight there (the flight ends at the surface, docs/VOLUME.md)
    o3 = VG.delta_track(grid, 1.0, 2.0, (-0.5, 0.5, 0.5), (1.0, 0.0, 0.0), 1.7, [11], log=8, dim=2)
    assert o3["kind"][0] == VG.KINDS["end"] and o3["steps"][0] == 3 and o3["s"][0] == np.float32(1.7)


# ---- 4. a constant grid is the homogeneous medium -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("majorant_scale", [1.0, 2.0])
@pytest.mark.parametrize("box", [False, True])
def test_a_constant_grid_is_the_homogeneous_medium_in_expectation(orc, box, majorant_scale):
    """constant_grid_slab at 32 x 32, 64 samples per pixel as 16 frames of 4: the mean film equals its homogeneous twin scene's
    within 4 standard errors of the difference (the frames' means are the samples), also with a diffuse box inside the slab.  Under
    EvalMajorant's majorant every collision is real and the two scenes draw the very same paths; under twice that, half the
    collisions are null and the agreement is statistical."""
    w = h = 32
    means = {}
    for grid in (True, False):
        fs, cam = _scene("constant_grid_slab", grid=grid, box=box, majorant_scale=majorant_scale)
        c = make_camera(orc, cam, w, h)
        seeds = orc.init_sampler(w, h, 0)
        v = VG.Volume()
        m = []
        for f in range(16):
            film = v.render(fs, c, seeds, w, h, spp=4, frame=f, progressive=False, break_on_terminate=False, max_depth=8)
            m.append(film[..., :3].astype(np.float64).mean())
        assert v.counters["flight_capped"] == 0 and v.counters["connection_capped"] == 0
        means[grid] = np.asarray(m)
    d = means[True].mean() - means[False].mean()
    se = np.sqrt(means[True].var(ddof=1) / 16 + means[False].var(ddof=1) / 16)
    print("box %s majorant x %g: grid %.5f homogeneous %.5f, difference %.2g = %.2f standard errors" % (box, majorant_scale, means[True].mean(), means[False].mean(), d, d / max(se, 1e-30)))
    assert 0.05 < means[False].mean() < 1.05
    assert abs(d) <= 4 * se


def test_a_constant_grid_is_the_homogeneous_medium_with_the_light_inside_the_fog(orc):
    """constant_grid_slab with an area light inside the slab, a black background and the diffuse box, under EvalMajorant's majorant:
    the two scenes draw the same paths, but every connection to the light is ratio-tracked through the grid (0 or 1 per walk, ending
    inside the medium) where the homogeneous scene multiplies exp(-sigma * distance).  The mean films agree within 4 standard
    errors of the difference (32 x 32, 64 samples per pixel as 16 frames of 4)."""
    w = h = 32
    means, tracked = {}, 0
    for grid in (True, False):
        fs, cam = _scene("constant_grid_slab", grid=grid, box=True, light=True, bg=(0.0, 0.0, 0.0))
        c = make_camera(orc, cam, w, h)
        seeds = orc.init_sampler(w, h, 0)
        v = VG.Volume()
        m = []
        for f in range(16):
            film = v.render(fs, c, seeds, w, h, spp=4, frame=f, progressive=False, break_on_terminate=False, max_depth=8)
            m.append(film[..., :3].astype(np.float64).mean())
        assert v.counters["connections"] > 1000 and v.counters["connection_capped"] == 0
        means[grid] = np.asarray(m)
    _, st = VG.Volume().render(*_light_case(orc, w, h), frame=0, capture=1)
    assert st["conn"]["track_steps"].sum() > 50        # connections are tracked through the grid
    d = means[True].mean() - means[False].mean()
    se = np.sqrt(means[True].var(ddof=1) / 16 + means[False].var(ddof=1) / 16)
    print("light inside: grid %.5f homogeneous %.5f, difference %.2g = %.2f standard errors" % (means[True].mean(), means[False].mean(), d, d / se))
    assert means[False].mean() > 0.01 and se > 0
    assert abs(d) <= 4 * se


def _light_case(orc, w, h):
    fs, cam = _scene("constant_grid_slab", grid=True, box=True, light=True, bg=(0.0, 0.0, 0.0))
    return fs, make_camera(orc, cam, w, h), orc.init_sampler(w, h, 0), w, h


# ---- 5. the gates the GPU tests rest on ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(64, 48), (100, 52)])
@pytest.mark.parametrize("name", ["cornell_box_smoke_grid", "smoke_grid_ragged"])
def test_the_gates_of_the_gpu_tests(orc, name, size):
    """Frames 0-2, after iterations 0, 1 and 3: the twin alone marks at most 0.5 % of the pixels as near ties, both cap counters and
    the stack and walk overflow counters are zero, and the scene does what it was built for: flights with null collisions, events,
    flights that reach their end, rays that miss the grid's box, connections tracked through the grid."""
    w, h = size
    fs, cam = _scene(name)
    c = make_camera(orc, cam, w, h)
    seeds = orc.init_sampler(w, h, 0)
    seen = dict(events=0, ends=0, null=0, missed=0, tracked=0)
    for f in range(3):
        for it in (0, 1, 3):
            v = VG.Volume()
            _, st = v.render(fs, c, seeds, w, h, frame=f, capture=it)
            assert (st["ties"] != 0).mean() <= 0.005, (f, it, (st["ties"] != 0).mean())
            assert v.counters["flight_capped"] == 0 and v.counters["connection_capped"] == 0
            assert v.counters["stack_overflow"] == 0 and v.counters["walk_overflow"] == 0
            s = st["state"]
            in_medium = s["hit"] & (s["stack_size"] > 0) & ~s["terminated"]
            seen["events"] += int(s["scattered"].sum())
            seen["ends"] += int((s["sampled"] & ~s["scattered"]).sum())
            seen["null"] += int((s["flight_steps"] > 1).sum())
            seen["missed"] += int((in_medium & ~s["sampled"] & ~s["passed"]).sum())
            seen["tracked"] += int(st["conn"]["track_steps"].sum())
    print(name, size, seen)
    assert seen["events"] > 300 and seen["ends"] > 300 and seen["null"] > 100 and seen["tracked"] > 300
    if name == "smoke_grid_ragged":
        assert seen["missed"] > 50
    for spp, brk in ((1, True), (2, False)):
        v = VG.Volume()
        for f in range(3):
            v.render(fs, c, seeds, w, h, spp=spp, frame=f, break_on_terminate=brk)
            assert v.counters["flight_capped"] == 0 and v.counters["connection_capped"] == 0


# ---- 6. the builder's bytes ---------------------------------------------------------------------------------------------------------------
def test_builder_bytes():
    from aten_amd.scene.builder import SceneBuilder
    a, b = SceneBuilder(), SceneBuilder()
    ia = a.add_medium_material("m", -0.4, 0.0, 0.5, (1.0, 0.0, 0.0))
    ib = b.add_medium_material("m", -0.4, 0.0, 0.5, (1.0, 0.0, 0.0), grid=None, majorant=None)
    assert a.materials[ia][1].tobytes() == b.materials[ib][1].tobytes()
    assert a.materials[ia][1]["medium"].tobytes() == struct.pack("<fffif3f", -0.4, 0.0, 0.5, -1, -1.0, 1.0, 0.0, 0.0)
    g = b.add_grid(np.array([[[0.25, 0.75], [0.5, 0.125]]], np.float32), (0.0, 0.0, 0.0), 1.0)
    ig = b.add_medium_material("g", 0.3, 0.0, 3.0, (0.0, 0.0, 0.0), grid=g)
    assert b.materials[ig][1]["medium"].tobytes() == struct.pack("<fffif3f", 0.3, 0.0, 3.0, g, 3.0 * 0.75, 0.0, 0.0, 0.0)      # EvalMajorant
    ih = b.add_medium_material("h", 0.3, 0.0, 3.0, (0.0, 0.0, 0.0), grid=g, majorant=5.0)
    assert b.materials[ih][1]["medium"].tobytes() == struct.pack("<fffif3f", 0.3, 0.0, 3.0, g, 5.0, 0.0, 0.0, 0.0)
    assert b.materials[ig][1]["is_medium"] == 1 and b.materials[ig][1]["attrib"] == 0
    fs, _ = _scene("cornell_box_smoke_grid")
    assert len(fs.grids) == 1 and fs.grids[0][0].shape == (8, 8, 8) and fs.grids[0][0].min() == 0.0 and fs.grids[0][0].max() == 1.0
