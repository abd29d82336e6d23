"""The production trace kernels held to float64 alone (tests/brute_force.py; docs/TRACE_GROUND_TRUTH.md): PathTracing.trace_closest and
PathTracing.trace_shadow against Moeller-Trumbore over every world-space triangle -- no oracle, no second walk of the same tree.

Per case of tests/brute_force_cases.py, on decided rays: object, triangle and hit-or-miss equal float64's, nothing excluded, and t, a, b
lie within 4 x what the ORACLE was measured to differ from float64 (profiles/parity_brute_force.jsonl, recorded by
tests/test_brute_force_cpu.py); on undecided rays the answer is a member of the candidate set; at most 3 % of a set is undecided.
Every case runs under the walk its tree calls for ("own") and under the lane-refilling walk ("refill"); node images small enough for
the LDS copy also with ATEN_AMD_LDS_NODES=0 ("global").

Trees: host-built top layers over rigid instances (quads, and boxes whose local box is off-centre), the device-built top layer
(tlas_rebuild, block path and general path), non-rigid instances (expected rule "local"), the device LBVH (a deforming blob, a
clustered and a flat soup), the skinned tick without a box read-back, the host builder's and the imported tree over sponza_lod.

Instance matrices that ENLARGE (`double`, `nonuniform`, `shear`, host-built and `_dev`) are no case of that comparison: there the
reference's walk prunes the top layer's WORLD boxes with a t_max held in the instance's smaller LOCAL unit, and its answer depends on
its order -- neither rule.  The kernels restate the reference.  test_enlarging_matrices_stay_within_what_any_order_gives holds them to
what float64 can assert of any order (brute_force.any_order), and pins the number of decided rays off rule "local": over a host-built
top layer the oracle's own count (160 / 8 / 16 of 4 068, recorded by the CPU module), over the device-built one the recorded
165 / 4 / 15."""
import numpy as np
import pytest

import brute_force as B
import brute_force_cases as K
from test_gpu_shadow_rays import _ctx

pytestmark = pytest.mark.gpu

WALKS = ["own", "refill"]
_f64 = {}
_shadow = {}


def prepared(name, c, r):
    """(triangles, rays, float64 answers) of a case, computed once on the CPU (the skinned cases: from the vertices r holds)."""
    if name not in _f64:
        tris = c.tris(r) if c.tris is not None else B.world_triangles(c.host)
        if c.rays == "primary":
            from aten_amd.scene.camera import create_camera
            w, h = 96, 54           # (the CPU module walks 160 x 90; float64 over 22 082 triangles costs a second per 1 300 rays)
            r.updateCamera(create_camera(c.cam["pos"], c.cam["at"], c.cam["vfov"], w, h))
            r.initSampler(w, h, 0)
            rec = r.generate_paths(w, h, 0, 0)
            rays = B.Rays(rec["org"], rec["dir"], B.FLT_MAX, "primary")
            rays.dir = np.ascontiguousarray(rec["dir"])
        else:
            rays = c.ray_sets(tris)
        _f64[name] = (tris, rays, B.closest(tris, rays.org, rays.dir, B.EPS, rays.t_max, c.rule))
    return _f64[name]


@pytest.mark.parametrize("name,walk", [(n, w) for n in K.CLOSEST for w in WALKS + (["global"] if n in K.SMALL else [])])
def test_closest_hits_equal_float64(monkeypatch, name, walk):
    c = K.case(name)
    r = _ctx(monkeypatch, walk, c.upload)
    try:
        if c.tick is not None:
            c.tick(r)
        tris, rays, want = prepared(name, c, r)
        if c.rays == "sets":
            B.check_sets(rays, want.hit, want.decided, name)
        else:
            assert (~want.decided).mean() <= B.UNDECIDED_CAP
        hits = B.trace(lambda rec, lo, hi: r.trace_closest(rec, lo, hi), rays)
    finally:
        r.close()
    worst = B.compare(tris, rays, want, hits, c.rule, "%s, %s walk" % (name, walk))
    bound = B.float_bounds(name)
    print("%s, %s walk: t %.3g relative, a %.3g, b %.3g; bounds %.3g, %.3g, %.3g" % ((name, walk) + tuple(worst) + bound))
    for what, v, b in zip(("t (relative)", "a", "b"), worst, bound):
        assert v <= b, "%s, %s walk: %s is %.6g from float64, the bound is %.6g" % (name, walk, what, v, b)


@pytest.mark.parametrize("name,walk", [(n, w) for n in K.ANY_ORDER for w in WALKS + ["global"]])
def test_enlarging_matrices_stay_within_what_any_order_gives(monkeypatch, name, walk):
    c = K.case(name)
    r = _ctx(monkeypatch, walk, c.upload)
    try:
        if c.tick is not None:
            c.tick(r)
        tris, rays, want = prepared(name, c, r)
        hits = B.trace(lambda rec, lo, hi: r.trace_closest(rec, lo, hi), rays)
    finally:
        r.close()
    free = np.flatnonzero(rays.t_max == np.float32(B.FLT_MAX))
    ok = B.any_order(tris, rays.take(free), hits[free])
    assert ok.all(), "%s, %s walk: %d of %d rays, first %r" % (name, walk, int((~ok).sum()), len(free), np.flatnonzero(~ok)[:8].tolist())
    objid, tri_id, _ = B.canonical(tris, rays.org, rays.dir, hits, rays.t_max, c.rule)
    off = int((want.decided & ~want.in_candidates(tris, objid, tri_id)).sum())
    print("%s, %s walk: %d decided rays off rule local" % (name, walk, off))
    kind, key = ("order_dependence_device", "decided_off_rule_local") if name.endswith("_dev") else ("order_dependence", "decided_off_rule_local")
    rec = [x for x in B.read_records() if x["record"] == kind and x["case"] == name]
    assert rec, "profiles/parity_brute_force.jsonl has no %s record for %s (measured now: %d)" % (kind, name, off)
    assert off == rec[0][key], "%s, %s walk: %d decided rays off rule local, recorded %d" % (name, walk, off, rec[0][key])


@pytest.mark.parametrize("walk", WALKS)
@pytest.mark.parametrize("twin", [0, 2])
@pytest.mark.parametrize("name", K.SHADOW)
def test_shadow_verdicts_equal_float64(monkeypatch, name, twin, walk):
    """trace_shadow towards a point light, flavours fused and counted, with and without any-hit twin trees: the verdict of every decided
    ray is float64's under the case's rule (scaled instances: the blocker's LOCAL t against the world distance to the light)."""
    c = K.case(name)
    li, pos = K.point_light(c.host)
    if name not in _shadow:
        tris = B.world_triangles(c.host)
        o, d, dist = c.shadow_set(tris, pos)
        _shadow[name] = (o, d, dist) + B.visible(tris, o, d, dist, c.rule)
    o, d, dist, vis, dec = _shadow[name]
    B.check_verdicts(vis, dec, name)
    r = _ctx(monkeypatch, walk, c.host, anyhit_twin=twin)
    try:
        assert (r.anyhit_twins() > 0) == (twin == 2)
        for flavour in ("fused", "counted"):
            got = r.trace_shadow(o, d, dist, li, flavour=flavour).astype(bool)
            bad = np.flatnonzero((got != vis) & dec)
            assert len(bad) == 0, ("%s, %s walk, twins %d, %s: %d of %d decided verdicts differ from float64, first %r"
                                   % (name, walk, twin, flavour, len(bad), int(dec.sum()), bad[:8].tolist()))
    finally:
        r.close()
