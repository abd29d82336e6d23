"""The oracle's shade-stage twin (orc.shade_stage: PathTracing::shade / ShadeMiss once per vertex) is the oracle's own loop and not a near
copy of it: fed with what orc.record_vertices saw in front of every vertex of a frame, its outputs chain into the next bounce's
recorded inputs bit for bit, and its contributions -- plus the shadow rays' where orc.shadow_visible says visible -- close to
orc.render's film byte for byte.  Then the floors of the vertex sets the GPU gate runs on (tests/shade_vertices.py)."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import shade_vertices as V

from aten_amd import layout as L

F_TERMINATED, F_SINGULAR, F_HIT = 1, 2, 4
LIGHT_MASK, STENCIL_BIT = 0x3fffffff, 0x40000000


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def shadow_added(orc, fs, res):
    """lightcontrib [n, 3] of the results with a shadow ray the oracle's HitTestToTargetLight lets through, zero elsewhere."""
    add = np.zeros((len(res), 3), np.float32)
    s = np.flatnonzero(res["has_shadow"] != 0)
    if len(s):
        q = orc.shadow_queries(res["sh_o"][s], res["sh_d"][s], res["sh_dist"][s], (res["light_bits"][s] & LIGHT_MASK).astype(np.int32),
                               (res["light_bits"][s] & STENCIL_BIT) != 0)
        vis = orc.shadow_visible(fs, q).astype(bool)
        add[s[vis]] = res["sh_c"][s[vis]]
    return add


def sample_epilogue(contrib):
    """One sample per pixel, not progressive (pathtracing.cpp:339-366): an invalid colour is skipped, so 0 / 0; else colour / 1; w = 1."""
    c = np.ascontiguousarray(contrib, np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        bad = (~np.isfinite(c)).any(-1) | (c < 0).any(-1)
        col = np.where(bad[..., None], np.float32(0.0), c)
        cnt = np.where(bad, np.float32(0.0), np.float32(1.0))
        film = np.concatenate([col / cnt[..., None], np.ones(c.shape[:-1] + (1,), np.float32)], -1)
    return film.astype(np.float32)


@pytest.mark.parametrize("name", V.CLOSURE_SETS)
def test_outputs_chain_into_the_next_bounce_and_the_film_closes(orc, cornell, sponza_disney, name):
    vs = V.build(orc, name, cornell, sponza_disney)
    recorded = [b for b in vs.batches if b.label == "recorded"]
    assert [b.bounce for b in recorded] == list(range(len(recorded)))
    final = np.full((vs.h * vs.w, 3), np.nan, np.float32)
    assert len(recorded[0]) == vs.w * vs.h
    for k, b in enumerate(recorded):
        res = b.want
        total = (res["contrib"] + shadow_added(orc, vs.fs, res)).astype(np.float32)       # HitShadowRay: path.contrib += lightcontrib
        on = res["goes_on"] != 0
        nxt = recorded[k + 1] if k + 1 < len(recorded) else None
        assert on.sum() == (len(nxt) if nxt is not None else 0)
        final[b.rec["pixel"][~on]] = total[~on]
        if nxt is None:
            continue
        # ---- outputs chain into inputs: same pixels in the same order, every field but the hit record bit-equal
        assert np.array_equal(b.rec["pixel"][on], nxt.rec["pixel"])
        r = res[on]
        for got, want in ((r["org"], nxt.rec["org"]), (r["pdfb"], nxt.rec["pdfb"]), (r["dir"], nxt.rec["dir"]),
                          (r["throughput"], nxt.rec["throughput"]), (total[on], nxt.rec["contrib"])):
            assert np.array_equal(bits(got), bits(want))
        assert np.array_equal(r["dimension"], nxt.rec["dimension"])
        assert np.array_equal(r["flags"] & ~np.uint32(F_HIT), nxt.rec["flags"])
        assert np.all(r["flags"] & F_HIT) and not np.any(r["flags"] & F_TERMINATED)
        # ---- ... and the hit record is the closest hit of that ray
        rays = np.zeros(len(r), L.RAY); rays["org"] = r["org"]; rays["dir"] = r["dir"]
        hit, _ = orc.trace_closest(vs.fs, rays)
        is_hit = hit["objid"] >= 0
        assert np.array_equal(is_hit, nxt.rec["objid"] >= 0)
        for f in ("objid", "tri_id"):
            assert np.array_equal(hit[f][is_hit], nxt.rec[f][is_hit])
        for f in ("a", "b"):
            assert np.array_equal(bits(hit[f][is_hit]), bits(nxt.rec[f][is_hit]))
    # ---- the film closes: every pixel's last vertex, the epilogue in NumPy
    final = final.reshape(vs.h, vs.w, 3)
    assert np.array_equal(bits(final), bits(vs.contrib[..., :3]))
    film = orc.render(vs.fs, vs.cam, vs.seeds, vs.w, vs.h, vs.depth, vs.rr, 1, 0, progressive=False)
    assert np.array_equal(bits(sample_epilogue(final)), bits(film))


def test_unobserved_fields_are_zero_and_bad_calls_are_refused(orc, cornell):
    vs = V.build(orc, "cornell", cornell)
    for b in vs.batches:
        r = b.want
        off = r["goes_on"] == 0
        for f in ("org", "dir", "throughput", "pdfb", "dimension"):
            assert not np.any(bits(r[f][off]) if r[f].dtype == np.float32 else r[f][off])
        ns = r["has_shadow"] == 0
        for f in ("sh_o", "sh_d", "sh_c", "sh_dist"):
            assert not np.any(bits(r[f][ns]))
        assert not np.any(r["light_bits"][ns]) and not np.any(r["sh_c_w"][ns])
        assert np.array_equal(r["light_bits"], r["sh_c_w"])
        assert not np.any((r["goes_on"] != 0) & ((r["flags"] & F_TERMINATED) != 0))
        assert not np.any((r["has_shadow"] != 0) & ((r["flags"] & F_TERMINATED) != 0))
    b = vs.batches[0]
    args = (vs.fs, vs.cam, vs.seeds)
    assert len(orc.shade_stage(*args, b.rec[:0], vs.w, vs.h, 0, vs.depth, vs.rr)) == 0
    with pytest.raises(ValueError):
        orc.shade_stage(*args, b.rec[:4], vs.w, vs.h, vs.depth, vs.depth, vs.rr)          # a bounce at max_depth
    with pytest.raises(ValueError):
        orc.shade_stage(*args, b.rec[:4], vs.w, vs.h, 0, vs.depth, vs.rr, flavour="lookahead")  # not served
    for field, value in (("pixel", vs.w * vs.h), ("pixel", -1), ("flags", F_TERMINATED), ("tri_id", 1 << 30)):
        bad = b.rec[:4].copy()
        hit = int(np.flatnonzero(bad["objid"] >= 0)[0])
        bad[field][hit] = value
        with pytest.raises(ValueError):
            orc.shade_stage(*args, bad, vs.w, vs.h, 0, vs.depth, vs.rr)


def test_every_category_keeps_its_floor_behind_the_margin_rule(orc, cornell, sponza_disney):
    sets = [V.build(orc, n, cornell, sponza_disney) for n in V.SETS]
    counts = V.check_floor(sets)
    assert set(counts) == set(orc.SHADE_CATEGORIES)
    # the hand-built vertices no frame produces are there, in the set that carries them
    labels = {b.label for b in V.build(orc, "cornell", cornell).batches}
    assert {"zero throughput", "NaN throughput", "other side", "grazing", "pdfb 0 at a miss"} <= labels
    # between them the sets compile all five material sets and every light type
    for light in ("nee_point", "nee_spot", "nee_direction", "nee_area", "nee_ibl"):
        assert counts[light] >= V.FLOOR


def test_the_kept_findings_are_ill_conditioned_in_the_oracle_itself(orc):
    """The vertices whose pdf the kernel misses by per cent (shade_vertices.FINDINGS): one ulp of the incoming direction moves the
    oracle's OWN pdf by more than 1 % at each of them, and by less than 1e-5 at the ordinary vertices next to them."""
    for name in V.FINDINGS:
        vs = V.build(orc, name)
        kept = [b for b in vs.batches if b.label == "finding"]
        assert len(kept) == len(V.FINDINGS[name])
        for b in kept:
            assert b.want["goes_on"][0] and V.ill_conditioning(vs, b, np.array([0]), "pdfb")[0] > 1e-2, (name, b.bounce)
        rec = [b for b in vs.batches if b.label == "recorded" and b.bounce == 1][0]
        on = np.flatnonzero(rec.compared & (rec.want["goes_on"] != 0))
        assert np.median(V.ill_conditioning(vs, rec, on, "pdfb")) < 1e-5


def scene_blob(fs, cam, seeds, w, h, depth, rr):
    """The flat arrays behind an atn_scene_desc as oracle/shade_driver.cpp reads them."""
    a = fs.arrays
    tex = [np.ascontiguousarray(t, np.float32) for t in a["textures"]]
    head = [0x534e5441, w, h, depth, rr, len(a["objects"]), len(a["matrices"]), len(a["materials"]), len(a["lights"]), len(a["triangles"]),
            len(a["vtx_pos"]), len(a["bvh_lists"]), len(tex), len(seeds)]
    parts = [struct.pack("<14I", *head), struct.pack("<%dI" % len(a["bvh_lists"]), *[len(n) for n in a["bvh_lists"]]),
             b"".join(struct.pack("<2i", t.shape[1], t.shape[0]) for t in tex),
             C.string_at(C.addressof(fs.desc.config), C.sizeof(fs.desc.config)),
             struct.pack("<6f", *(list(fs.desc.scene_bbox_min) + list(fs.desc.scene_bbox_max))), cam.tobytes()]
    for k in ("objects", "matrices", "materials", "lights", "triangles", "vtx_pos", "vtx_nml"):
        parts.append(np.ascontiguousarray(a[k]).tobytes())
    parts += [np.ascontiguousarray(n).tobytes() for n in a["bvh_lists"]] + [t.tobytes() for t in tex]
    parts.append(np.ascontiguousarray(seeds, np.uint32).tobytes())
    return b"".join(parts)


def test_the_entries_run_clean_under_asan_and_ubsan_in_a_program_of_their_own(tmp_path, orc, cornell):
    """oracle/shade_driver.cpp -- the oracle's unit compiled into a stand-alone program with -fsanitize=address,undefined -- records the
    Cornell box's vertices, shades every bounce, chains them and tries the refusals: exit status 0 and no sanitizer report."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    vs = V.build(orc, "cornell", cornell)
    blob = tmp_path / "cornell.blob"
    blob.write_bytes(scene_blob(vs.fs, vs.cam, vs.seeds, vs.w, vs.h, vs.depth, vs.rr))
    b = subprocess.run(["make", "-C", os.path.join(root, "oracle"), "shade_driver_san", "OUT=%s" % tmp_path], capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    env = dict(os.environ, OMP_NUM_THREADS="4", ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(tmp_path / "shade_driver_san"), str(blob)], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    recorded = sum(len(x) for x in vs.batches if x.label == "recorded")
    assert "ok: %d vertices" % recorded in r.stdout, r.stdout
