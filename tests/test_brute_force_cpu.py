"""The oracle held to a float64 brute force over every world-space triangle (tests/brute_force.py; docs/TRACE_GROUND_TRUTH.md): here the
reference's rule shows that it passes by itself, on the CPU, before tests/test_gpu_brute_force.py holds the device walks to the same
float64 answers without the oracle.

For every scene of tests/brute_force_cases.py and every ray set: orc.trace_closest equals rule "local" on EVERY decided ray (object,
triangle, hit or miss), stays inside the candidate set on the others, and at most 3 % of a set is undecided.  The largest distance between
the oracle's t, a, b and float64's is measured and held to profiles/parity_brute_force.jsonl (ATEN_BRUTE_FORCE_RECORD=1 rewrites the
file); the GPU module takes 4 x those values as its float bound.  Two seeded faults (a shrunk box, an unlinked leaf) must be noticed.
Rules "world" and "local" agree under rigid matrices and part under scaled ones; the shares are recorded.

Matrices that ENLARGE (`double`, `nonuniform`, `shear`: |W2L d| < 1 for some d) are no case of that comparison: there the reference
follows neither rule, and that is pinned here on the oracle: the reference prunes the top layer's WORLD boxes with a t_max held in the hit
instance's smaller LOCAL unit, a nearer instance is culled once a farther one has been hit, and the answer depends on the order of the
walk -- test_enlarging_matrices_make_the_answer_depend_on_the_order (decided rays off rule "local", of 4 068: 160 / 8 / 16) and
test_enlarging_matrices_stay_within_what_any_order_gives."""
import json
import os

import numpy as np
import pytest

import brute_force as B
import brute_force_cases as K
from conftest import make_camera

_state = {}
_records = {}
RECORD = os.environ.get("ATEN_BRUTE_FORCE_RECORD") == "1"


def prepared(orc, name):
    """(case, triangles, rays, float64 answers under the case's rule), built once."""
    if name not in _state:
        c = K.case(name)
        tris = B.world_triangles(c.host)
        if c.rays == "primary":
            cam = make_camera(orc, c.cam, 160, 90)
            rec = orc.generate_paths(cam, orc.init_sampler(160, 90, 0), 160, 90, 0, 0)
            rays = B.Rays(rec["org"], rec["dir"], B.FLT_MAX, "primary")
            rays.dir = np.ascontiguousarray(rec["dir"])
        else:
            rays = c.ray_sets(tris)
        want = B.closest(tris, rays.org, rays.dir, B.EPS, rays.t_max, c.rule)
        _state[name] = (c, tris, rays, want)
    return _state[name]


def oracle_hits(orc, fs, rays):
    return B.trace(lambda r, lo, hi: orc.trace_closest(fs, r, lo, hi)[0], rays)


def note(record, key, **values):
    _records[(record, key)] = dict(record=record, case=key, **values)


@pytest.mark.parametrize("name", K.CLOSEST)
def test_oracle_equals_float64_on_every_decided_ray(orc, name):
    c, tris, rays, want = prepared(orc, name)
    if c.rays == "sets":
        B.check_sets(rays, want.hit, want.decided, name)
    else:
        assert (~want.decided).mean() <= B.UNDECIDED_CAP
    trees = [("host tree", c.host)]
    if hasattr(c, "lbvh"):      # the device rebuilds this list as an LBVH: its CPU twin is walked too
        fresh = K.MAKERS[name]()
        trees.append(("LBVH twin", K.host_with_lbvh(fresh.host, c.lbvh, orc.lbvh_build)))
    worst = np.zeros(3)
    for what, fs in trees:
        worst = np.maximum(worst, B.compare(tris, rays, want, oracle_hits(orc, fs, rays), c.rule, "%s, %s" % (name, what)))
    print("%s: %d rays, %.4f undecided, oracle vs float64: t %.3g relative, a %.3g, b %.3g" % ((name, len(rays), (~want.decided).mean()) + tuple(worst)))
    note("float_bound", name, rule=c.rule, rays=len(rays), undecided=float((~want.decided).mean()),
         t_rel=float(worst[0]), a_abs=float(worst[1]), b_abs=float(worst[2]))
    if not RECORD:
        have = [r for r in B.read_records() if r.get("record") == "float_bound" and r["case"] == name]
        assert have, "profiles/parity_brute_force.jsonl has no float bound for %s" % name
        for k, v in zip(("t_rel", "a_abs", "b_abs"), worst):
            assert v <= have[0][k] * 1.001 + 1e-12, "%s: %s measured %.6g, recorded %.6g" % (name, k, v, have[0][k])


def _unlink(nodes, k):
    nxt = nodes["miss"][k]
    for f in ("hit", "miss"):
        nodes[f][nodes[f] == np.float32(k)] = nxt


def test_a_shrunk_box_and_an_unlinked_leaf_are_noticed(orc):
    """In copies of a host-built scene: (a) the root box of the boxes' bottom-level list shrinks by 10 % about its centre in the oracle's
    input, (b) the leaf of the triangle that wins the most rays is linked out of that list.  Either must show as decided-ray mismatches."""
    c, tris, rays, want = prepared(orc, "box7")
    B.compare(tris, rays, want, oracle_hits(orc, c.host, rays), c.rule, "box7 intact")
    # (a)
    fs = K.MAKERS["box7"]().host
    nodes = fs.arrays["bvh_lists"][1].copy()
    assert nodes["f0"][0] < 0 and nodes["f1"][0] < 0          # an inner node
    mid, half = 0.5 * (nodes["boxmin"][0] + nodes["boxmax"][0]), 0.5 * (nodes["boxmax"][0] - nodes["boxmin"][0])
    nodes["boxmin"][0], nodes["boxmax"][0] = mid - 0.9 * half, mid + 0.9 * half
    fs.replace_bvh_list(1, nodes)
    with pytest.raises(AssertionError, match=r"of them decided") as e:
        B.compare(tris, rays, want, oracle_hits(orc, fs, rays), c.rule, "box7 shrunk")
    assert " (0 of them decided)" not in str(e.value)
    # (b)
    fs = K.MAKERS["box7"]().host
    nodes = fs.arrays["bvh_lists"][1].copy()
    top = np.bincount(want.tri_id[want.hit & want.decided]).argmax()
    leaves = np.flatnonzero((nodes["f1"] == np.float32(top)) & (nodes["f2"] < 0))
    assert len(leaves) >= 1
    for k in leaves:
        _unlink(nodes, int(k))
    fs.replace_bvh_list(1, nodes)
    with pytest.raises(AssertionError, match=r"of them decided") as e:
        B.compare(tris, rays, want, oracle_hits(orc, fs, rays), c.rule, "box7 unlinked")
    assert " (0 of them decided)" not in str(e.value)


@pytest.mark.parametrize("name", [n for n in K.ANY_ORDER if not n.endswith("_dev")])
def test_enlarging_matrices_make_the_answer_depend_on_the_order(orc, name):
    """On the oracle, decided rays differ from rule "local"; their count is recorded, and the device module holds the kernels to the
    same count over the same top layer (and to its own record over the device-built one, which threads the instances differently)."""
    c, tris, rays, want = prepared(orc, name)
    hits = oracle_hits(orc, c.host, rays)
    objid, tri_id, _ = B.canonical(tris, rays.org, rays.dir, hits, rays.t_max, c.rule)
    off = int((want.decided & ~want.in_candidates(tris, objid, tri_id)).sum())
    print("%s: %d decided rays off rule local" % (name, off))
    assert off > 0
    note("order_dependence", name, rays=len(rays), decided_off_rule_local=off)


@pytest.mark.parametrize("name", K.ANY_ORDER)
def test_enlarging_matrices_stay_within_what_any_order_gives(orc, name):
    """Where rule "local" does not describe the reference (docs/TRACE_GROUND_TRUTH.md), the walk's answer still is a real hit that no
    unskippable nearer hit beats: brute_force.any_order."""
    c, tris, rays, _ = prepared(orc, name)
    free = rays.take(np.flatnonzero(rays.t_max == np.float32(B.FLT_MAX)))
    ok = B.any_order(tris, free, oracle_hits(orc, c.host, free))
    assert ok.all(), "%s: %d of %d rays, first %r" % (name, int((~ok).sum()), len(free), np.flatnonzero(~ok)[:8].tolist())


def _differ(tris, rays, a, b):
    both = a.decided & b.decided
    diff = both & ((a.hit != b.hit) | (a.hit & b.hit & (tris.klass[a.tindex] != tris.klass[b.tindex])))
    return int(diff.sum()), int(both.sum())


@pytest.mark.parametrize("name", K.CLOSEST + list(K.ENLARGING))
def test_rules_agree_under_isometries_and_part_under_scales(orc, name):
    c, tris, rays, want = prepared(orc, name)
    other = B.closest(tris, rays.org, rays.dir, B.EPS, rays.t_max, "world" if c.rule == "local" else "local")
    n, both = _differ(tris, rays, want, other)
    print("%s: rules differ on %d of %d rays decided under both" % (name, n, both))
    if name in K.RIGID or name.startswith("mirror"):      # (a mirror keeps lengths: |W2L d| = 1)
        assert n == 0
    elif name == "atrium":
        share = n / both
        assert share >= 0.05, "the premise: the rules part on at least 5 %% of the atrium's primary rays, measured %.4f" % share
        note("rule_share", "atrium closest hits", rays=both, differ=n, share=share)
    else:
        assert n > 0
        note("rule_share", name + " closest hits", rays=both, differ=n, share=n / both)


def test_atrium_shadow_verdicts_under_both_rules(orc):
    """Shadow rays from surface points (the oracle's hits of a 64 x 36 frame and of one bounce, tests/shadow_rays.py category A's
    origins) towards a point just under the atrium's lamp: the share of verdicts that the local-unit rule moves, recorded."""
    import shadow_rays as S
    c, tris, _, _ = prepared(orc, "atrium")
    p, n = S.surface_points(orc, c.host, c.cam)
    o = orc.ray_offset(p, n)
    lamp = np.array([0.0, 5.55, 0.0])
    d = lamp[None, :] - o
    dist = np.linalg.norm(d, axis=1)
    vw, dw = B.visible(tris, o, d, dist, "world")
    vl, dl = B.visible(tris, o, d, dist, "local")
    both = dw & dl
    differ = int((vw != vl)[both].sum())
    assert both.mean() >= 1 - B.UNDECIDED_CAP
    print("atrium shadow verdicts: %d of %d differ between the rules" % (differ, int(both.sum())))
    # (a measurement, no premise: the statues stand on the floor, a blocker among them lies in the first quarter of a ray to the lamp,
    # and 2.2 times its distance is still short of the lamp.  test half_light holds the rule where it moves verdicts)
    note("rule_share", "atrium shadow verdicts", rays=int(both.sum()), differ=differ, share=differ / int(both.sum()))


@pytest.mark.parametrize("name", K.SHADOW)
def test_oracle_shadow_verdicts_equal_float64(orc, name):
    """The oracle's verdicts equal float64's under the case's rule on every decided ray -- and the set can tell: at least FLOOR of the
    decided verdicts flip when the stepped dist is replaced by the full distance to the light (a walk that ignored dist would be
    noticed), and on the scaled scene at least FLOOR flip between rule "local" and rule "world" (so would one that compared a world t)."""
    c = K.case(name)
    tris = B.world_triangles(c.host)
    li, pos = K.point_light(c.host)
    o, d, dist = c.shadow_set(tris, pos)
    vis, dec = B.visible(tris, o, d, dist, c.rule)
    B.check_verdicts(vis, dec, name)
    got = orc.shadow_visible(c.host, orc.shadow_queries(o, d, dist, li)).astype(bool)
    bad = np.flatnonzero((got != vis) & dec)
    assert len(bad) == 0, "%s: %d decided verdicts differ, first %r" % (name, len(bad), bad[:8].tolist())
    full = np.linalg.norm(d.astype(np.float64), axis=1).astype(np.float32)
    vf, df = B.visible(tris, o, d, full, c.rule)
    both = dec & df
    by_dist = float((vis != vf)[both].mean())
    print("%s: %.3f of %d decided verdicts flip between the stepped and the full dist" % (name, by_dist, int(both.sum())))
    note("shadow_share", name + " stepped vs full dist", rays=int(both.sum()), share=by_dist)
    if name != "sponza_sbvh_light":      # (a closed hall seen from its own surfaces: most blockers are near the origin; 3 % measured)
        assert by_dist >= B.FLOOR
    else:
        assert by_dist > 0.0
    if c.rule == "local":
        vw, dw = B.visible(tris, o, d, dist, "world")
        both = dec & dw
        by_rule = float((vis != vw)[both].mean())
        print("%s: %.3f of %d decided verdicts flip between the rules" % (name, by_rule, int(both.sum())))
        note("shadow_share", name + " local vs world", rays=int(both.sum()), share=by_rule)
        assert by_rule >= B.FLOOR


def test_a_hit_lost_to_the_perturbed_box_test_is_not_steady(orc):
    """The ray that made the steady criterion necessary (docs/TRACE_GROUND_TRUTH.md), replayed on box7: it enters a box on a
    triangle's border and leaves it 0.43 further on through the INTERIOR of another (m = 0.066), 3e-5 under a face it runs along at
    2.9e-6 rad.  The oracle's box test runs on dir + 1e-6 and reports a miss.  float64 hits that triangle well inside; PERTURB's model
    says the perturbed ray does not (not steady), so the ray is undecided and "miss" is a candidate.  With the model off
    (PERTURB = 0) the same ray would demand the hit: the oracle's answer would count as wrong."""
    c, tris, _, _ = prepared(orc, "box7")
    one = B.Rays(np.float32([[11.926553726196289, -1.5514891147613525, 2.562987804412842]]),
                 np.float32([[-0.9633311629295349, -0.023173052817583084, -0.2673126459121704]]), B.FLT_MAX, "replay")
    one.dir = np.float32([[-0.9633311629295349, -0.023173052817583084, -0.2673126459121704]])
    hits = oracle_hits(orc, c.host, one)
    assert hits["objid"][0] == -1
    want = B.closest(tris, one.org, one.dir, B.EPS, one.t_max, c.rule)
    assert want.hit[0] and not want.decided[0] and want.miss_ok[0]
    t, u, v = B.pairs(tris, one.org, one.dir, tris.index_of([3], [2]), c.rule)
    assert min(u[0], v[0], 1 - u[0] - v[0]) > 0.05 and abs(t[0] - 11.44) < 0.01
    B.compare(tris, one, want, hits, c.rule, "replay")
    keep = B.PERTURB
    try:
        B.PERTURB = 0.0
        strict = B.closest(tris, one.org, one.dir, B.EPS, one.t_max, c.rule)
        assert not strict.miss_ok[0]
        with pytest.raises(AssertionError):
            B.compare(tris, one, strict, hits, c.rule, "replay without the model")
    finally:
        B.PERTURB = keep


def test_zz_records(orc):
    """Last in the module: with ATEN_BRUTE_FORCE_RECORD=1 the measurements of this run replace profiles/parity_brute_force.jsonl;
    otherwise the file has a line for every measurement this run made."""
    if RECORD:
        kept = [r for r in B.read_records() if r["record"] == "order_dependence_device"]     # (measured by the device module)
        with open(B.records_path(), "w") as f:
            for k in sorted(_records):
                f.write(json.dumps(_records[k]) + "\n")
            for r in kept:
                f.write(json.dumps(r) + "\n")
        return
    have = {(r["record"], r["case"]) for r in B.read_records()}
    assert set(_records) <= have, sorted(set(_records) - have)


def test_spheres_are_refused():
    from aten_amd.scene import scenedefs
    fs, _ = scenedefs.cornell_box_variant(lights="sphere")
    with pytest.raises(ValueError, match="sphere"):
        B.world_triangles(fs)
