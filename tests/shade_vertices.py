"""Vertex sets for the per-vertex gate of the shade stage (tests/test_shade_stage_cpu.py, tests/test_gpu_shade_stage.py).

A set is one scene with the vertices of a small recorded frame -- orc.record_vertices: what the ORACLE's radiance loop hands shade /
ShadeMiss at every (pixel, bounce) -- plus hand-built vertices derived from them for the branches no frame reaches.  Vertices are kept
in BATCHES: one bounce, distinct pixels, so that a batch is one call of orc.shade_stage / PathTracing.shade_stage.  Every vertex
carries the category word and the decision margins the oracle reported for it (orc.SHADE_CATEGORIES, oracle/orc_pt.h DecisionLog).

The margin rule.  A vertex is left out of the GPU comparison when a branch decision that rests on a libm result (an NEE validity test,
PrepareForNextBounce's pdf / cosine test, a lobe pick behind sin / cos / pow) sat within MARGIN_ULPS = 4 float ulps of its threshold:
twice the <= 2 ulp difference between the two builds' math libraries that DESIGN.md section 4 states.  The ulp is that of the magnitude
the left side was summed from (1 for a cosine or a probability), not of the left side itself: a cosine of 1e-9 is millions of its own
ulps from 0 and still one rounding of a unit vector's component away from the other sign.  Decided from the oracle's margins alone,
on the CPU; no margin applies to decisions that rest on + - * / sqrt, min / max and CMJ draws -- those are exact on both sides."""
import numpy as np

from aten_amd import layout as L

F32 = np.float32
MARGIN_ULPS = 4.0
FLOOR = 32              # every category has at least this many compared vertices across the sets
MAX_EXCLUDED = 0.01     # no set leaves out more than this share of its vertices


class Batch:
    def __init__(self, label, bounce, rec):
        self.label, self.bounce, self.rec = label, int(bounce), np.ascontiguousarray(rec, L.SHADE_VERTEX)
        self.want = self.cat = self.margins = self.mtype = None

    def __len__(self):
        return len(self.rec)

    @property
    def compared(self):
        """The vertices the GPU comparison keeps: no libm decision within MARGIN_ULPS of its threshold."""
        return ~(self.margins[:, 0] <= MARGIN_ULPS)

    def has(self, name):
        from oracle import orc
        return ((self.cat >> orc.SHADE_CATEGORIES.index(name)) & 1).astype(bool)


class VertexSet:
    def __init__(self, name, fs, cam, seeds, w, h, depth, rr, ibl_importance, tier):
        self.name, self.fs, self.cam, self.seeds, self.w, self.h, self.depth, self.rr = name, fs, cam, seeds, w, h, depth, rr
        self.ibl_importance, self.tier = ibl_importance, tier
        self.flavour = "plain"
        self.batches = []
        self.contrib = None

    def oracle(self, orc, b):
        orc.set_sampling_options(ibl_importance=self.ibl_importance)
        try:
            b.want, b.cat, b.margins = orc.shade_stage(self.fs, self.cam, self.seeds, b.rec, self.w, self.h, b.bounce, self.depth, self.rr, flavour=self.flavour, details=True)
        finally:
            orc.set_sampling_options()
        tri = self.fs.arrays["triangles"]["mtrlid"][np.maximum(b.rec["tri_id"], 0)]
        b.mtype = np.where((b.rec["objid"] >= 0) & (tri >= 0), self.fs.arrays["materials"]["type"][np.maximum(tri, 0)], -1)
        return b

    @property
    def has_envmap(self):
        bg = self.fs.desc.config.bg
        return bg.envmap_tex_idx >= 0 and bg.enable_env_map != 0


def _hit_geometry(orc, vs, rec):
    """(p, n) of hit records: the oracle's evaluate_hit_result."""
    rays = np.zeros(len(rec), L.RAY); rays["org"] = rec["org"]; rays["dir"] = rec["dir"]
    isect = np.zeros(len(rec), L.INTERSECTION)
    for k in ("objid", "a", "b", "tri_id"):
        isect[k] = rec[k]
    isect["mtrlid"] = vs.fs.arrays["triangles"]["mtrlid"][rec["tri_id"]]
    ev = orc.evaluate_hits(vs.fs, rays, isect)
    return ev[:, 0:3].astype(F32), ev[:, 4:7].astype(F32)


def hand_built(orc, vs, base):
    """Batches derived from one recorded batch (same pixels, so each is a call of its own): the vertices no frame produces."""
    out = []
    rec = base.rec
    hit = np.flatnonzero(rec["objid"] >= 0)
    miss = np.flatnonzero(rec["objid"] < 0)
    if len(hit):
        z = rec[hit].copy(); z["throughput"] = 0.0
        out.append(Batch("zero throughput", base.bounce, z))
        q = rec[hit].copy(); q["throughput"][:, 1] = np.nan
        out.append(Batch("NaN throughput", base.bounce, q))
        p, n = _hit_geometry(orc, vs, rec[hit])
        # the same point met from the other side: back-facing hits of every material, the lamp's among them
        f = rec[hit].copy(); f["dir"] = -rec[hit]["dir"]; f["org"] = p + rec[hit]["dir"] * F32(0.25)
        out.append(Batch("other side", base.bounce, f))
        # an incoming direction within 1e-4 rad of the surface plane, on either side of it
        t = np.cross(n, np.where(np.abs(n[:, :1]) < 0.9, [[1.0, 0, 0]], [[0, 1.0, 0]])).astype(F32)
        t /= np.linalg.norm(t, axis=1, keepdims=True)
        ang = (np.linspace(-1e-4, 1e-4, len(hit)).astype(F32))[:, None]
        d = (t * np.cos(ang) - n * np.sin(ang)).astype(F32)
        d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)
        g = rec[hit].copy(); g["dir"] = d; g["org"] = (p - d * F32(0.25)).astype(F32)
        out.append(Batch("grazing", base.bounce, g))
    if len(miss) and base.bounce > 0:
        m = rec[miss].copy(); m["pdfb"] = 0.0
        out.append(Batch("pdfb 0 at a miss", base.bounce, m))
    return out


# ---- the sets ------------------------------------------------------------------------------------------------------------------------
def _variant(**kw):
    from aten_amd.scene import scenedefs
    return scenedefs.cornell_box_variant(**kw)


def _cornell_unregistered_lamp():
    """The Cornell box with the lamp's object taken off the light list's back reference (light_id = -1): an emissive surface that is no
    registered light, and triangles of the short box without a material (mtrlid = -1: the white-diffuse fallback)."""
    from aten_amd.scene import scenedefs
    fs, cam = scenedefs.cornell_box()
    fs.arrays["objects"]["light_id"][:] = -1
    tri = fs.arrays["triangles"]
    names = fs.names["materials"]
    tri["mtrlid"][tri["mtrlid"] == names.index("shortBox")] = -1
    return fs, cam


def _stencil_room():
    fs, cam = _variant(lights="point")
    mats, names = fs.arrays["materials"], fs.names["materials"]
    for n in names:
        mats["stencil_type"][names.index(n)] = 2 if n in ("shortBox", "tallBox") else 1
    return fs, cam


def _alpha_boxes():
    fs, cam = _variant(lights="area")
    mats, names = fs.arrays["materials"], fs.names["materials"]
    for n in ("shortBox", "tallBox"):
        mats["baseColor"][names.index(n)][3] = 0.5
    fs.desc.config.enable_alpha_blending = 1
    return fs, cam


def _scenedef(name, **kw):
    from aten_amd.scene import scenedefs
    return getattr(scenedefs, name)(**kw)


# name -> (factory, width, height, depth, rr_depth, ibl_importance, tier of the float bounds, hand-built batches from these bounces)
SETS = {
    "cornell": (None, 64, 64, 5, 3, False, "base", (0, 1, 4)),
    "point": (lambda: _variant(lights="point"), 64, 64, 5, 3, False, "base", ()),
    "spot": (lambda: _variant(lights="spot"), 64, 64, 5, 3, False, "base", ()),
    "directional": (lambda: _variant(lights="directional"), 64, 64, 5, 3, False, "base", ()),
    "area": (lambda: _variant(lights="area"), 64, 64, 5, 3, False, "base", ()),
    "extra": (lambda: _variant(extra_materials=True), 64, 64, 6, 3, False, "next", (1,)),
    "rough": (lambda: _variant(extra_materials="rough"), 64, 64, 6, 3, False, "next", ()),
    "retro": (lambda: _variant(extra_materials="retro"), 64, 64, 6, 3, False, "next", ()),
    "carpaint": (lambda: _variant(extra_materials="carpaint"), 64, 64, 6, 3, False, "next", ()),
    "many_light": (lambda: _scenedef("many_light_cornell"), 64, 64, 5, 3, False, "base", ()),
    "sponza_disney": ("sponza_disney", 64, 64, 5, 3, False, "base", ()),
    "atrium": (lambda: _scenedef("atrium", detail=0.25), 64, 64, 8, 3, False, "base", (4,)),
    "atrium_ibl": (lambda: _scenedef("atrium", detail=0.25), 64, 64, 8, 3, True, "base", ()),
    "toon": (lambda: _scenedef("toon_room"), 64, 64, 5, 3, False, "next", ()),
    "unregistered": (_cornell_unregistered_lamp, 64, 64, 5, 3, False, "base", (0,)),
    "stencil": (_stencil_room, 64, 64, 5, 3, False, "base", ()),
    "alpha": (_alpha_boxes, 64, 64, 5, 3, False, "base", ()),
}
CLOSURE_SETS = ("cornell", "sponza_disney")
# The findings of the GPU comparison, kept: vertices whose pdf the kernel misses by 0.8 % to 4.3 % (tests/test_gpu_shade_stage.py, the
# named cause).  (label, bounce, index in that batch) per set: copied into a batch of their own, "finding", so that they stay in the
# set whatever else changes; tests/test_shade_stage_cpu.py shows the cause on the CPU: one ulp of the incoming direction moves the
# ORACLE's own pdf by more than 1 % there.
FINDINGS = {"point": [("recorded", 2, 3210)], "area": [("recorded", 2, 298)],
            "atrium": [("recorded", 1, 1689), ("recorded", 2, 1073), ("recorded", 4, 436), ("other side", 4, 722), ("grazing", 4, 958)]}
_sets = {}


def build(orc, name, cornell=None, sponza_disney=None):
    """The set `name`, built once per session: recorded batches (one per bounce), then the hand-built ones."""
    if name in _sets:
        return _sets[name]
    make, w, h, depth, rr, ibl, tier, hand = SETS[name]
    fs, cam = cornell if make is None else sponza_disney if make == "sponza_disney" else make()
    c = orc.create_camera(cam["pos"], cam["at"], cam["vfov"], w, h)
    seeds = orc.init_sampler(w, h, 0)
    vs = VertexSet(name, fs, c, seeds, w, h, depth, rr, ibl, tier)
    vs.cam_dict = cam
    orc.set_sampling_options(ibl_importance=ibl)
    try:
        rec, bounce, vs.contrib = orc.record_vertices(fs, c, seeds, w, h, depth, rr)
    finally:
        orc.set_sampling_options()
    for b in range(depth):
        i = np.flatnonzero(bounce == b)
        if len(i):
            vs.batches.append(vs.oracle(orc, Batch("recorded", b, rec[i])))
    for b in [x for x in list(vs.batches) if x.bounce in hand]:
        vs.batches += [vs.oracle(orc, hb) for hb in hand_built(orc, vs, b)]
    for label, bounce, i in FINDINGS.get(name, ()):
        src = [x for x in vs.batches if x.label == label and x.bounce == bounce][0]
        vs.batches.append(vs.oracle(orc, Batch("finding", bounce, src.rec[i:i + 1])))
    _sets[name] = vs
    return vs


# The "svgf" flavour (SVGFRenderer::Shade / ShadeMiss with AOV spans): its loop differs from the path tracer's from the first vertex on
# -- the albedo is taken out where an AOV took it, and the last hit's "was Specular" travels as a flag --, so its vertices are chained
# through the svgf twin itself: bounce 0 from the recorded frame, every next bounce from the twin's outputs and orc.trace_closest.
# The reference's SVGF shade has no toon branch and no table-sampled environment: those sets stay with the plain flavour.
SVGF_SETS = ("cornell", "point", "extra", "carpaint", "sponza_disney", "atrium", "unregistered")
_svgf_sets = {}


def build_svgf(orc, name, cornell=None, sponza_disney=None):
    if name in _svgf_sets:
        return _svgf_sets[name]
    base = build(orc, name, cornell, sponza_disney)
    vs = VertexSet(name, base.fs, base.cam, base.seeds, base.w, base.h, base.depth, base.rr, False, base.tier)
    vs.cam_dict = base.cam_dict
    vs.flavour = "svgf"
    rec = [b for b in base.batches if b.label == "recorded" and b.bounce == 0][0].rec.copy()
    for bounce in range(vs.depth):
        b = vs.oracle(orc, Batch("chained", bounce, rec))
        vs.batches.append(b)
        on = b.want["goes_on"] != 0
        if not on.any():
            break
        r = b.want[on]
        rec = np.zeros(len(r), L.SHADE_VERTEX)
        for f in ("org", "dir", "pdfb", "throughput", "dimension"):
            rec[f] = r[f]
        rec["flags"] = r["flags"] & ~np.uint32(4)
        rec["pixel"] = b.rec["pixel"][on]
        rec["contrib"] = r["contrib"]       # (the shadow rays' light is left out: shade only adds to what it is given)
        rays = np.zeros(len(r), L.RAY); rays["org"] = r["org"]; rays["dir"] = r["dir"]
        hit, _ = orc.trace_closest(vs.fs, rays)
        miss = hit["objid"] < 0
        for f in ("objid", "a", "b", "tri_id"):
            rec[f] = hit[f]
        rec["objid"][miss] = -1; rec["tri_id"][miss] = -1; rec["a"][miss] = 0; rec["b"][miss] = 0
    _svgf_sets[name] = vs
    return vs


def ill_conditioning(vs, b, idx, field):
    """How far the oracle's own `field` moves, in the project's metric |d| / max(1, |value|), when one component of the incoming
    direction moves by one ulp: the largest of the six changes, per vertex of idx (inf where a decision flips)."""
    from oracle import orc
    out = np.zeros(len(idx))
    if len(idx) == 0:
        return out
    base = np.asarray(b.want[field][idx], np.float64).reshape(len(idx), -1)
    orc.set_sampling_options(ibl_importance=vs.ibl_importance)
    try:
        for c in range(3):
            for toward in (-10.0, 10.0):
                p = b.rec[idx].copy()
                p["dir"][:, c] = np.nextafter(p["dir"][:, c], np.float32(toward))
                w = orc.shade_stage(vs.fs, vs.cam, vs.seeds, p, vs.w, vs.h, b.bounce, vs.depth, vs.rr, flavour=vs.flavour)
                got = np.asarray(w[field], np.float64).reshape(len(idx), -1)
                with np.errstate(invalid="ignore"):
                    moved = (np.abs(got - base) / np.maximum(1.0, np.abs(base))).max(axis=1)
                moved = np.where(np.isnan(moved) | (w["goes_on"] != b.want["goes_on"][idx]), np.inf, moved)
                out = np.maximum(out, moved)
    finally:
        orc.set_sampling_options()
    return out


def category_counts(sets, compared_only=True):
    from oracle import orc
    n = np.zeros(len(orc.SHADE_CATEGORIES), np.int64)
    for vs in sets:
        for b in vs.batches:
            keep = b.compared if compared_only else np.ones(len(b), bool)
            for k in range(len(n)):
                n[k] += int((((b.cat >> k) & 1).astype(bool) & keep).sum())
    return dict(zip(orc.SHADE_CATEGORIES, n.tolist()))


def check_floor(sets):
    """Every category keeps FLOOR vertices after the margin rule, and no set loses more than MAX_EXCLUDED of its vertices to it."""
    for vs in sets:
        total = sum(len(b) for b in vs.batches)
        out = sum(int((~b.compared).sum()) for b in vs.batches)
        assert out <= MAX_EXCLUDED * total, "%s: the margin rule leaves out %d of %d vertices" % (vs.name, out, total)
    counts = category_counts(sets)
    short = {k: v for k, v in counts.items() if v < FLOOR}
    assert not short, "categories under the floor of %d: %r" % (FLOOR, short)
    return counts
