"""The per-vertex gate of the shade stage: every vertex of the sets in tests/shade_vertices.py through ONE launch of the production shade
kernel (PathTracing.shade_stage -> atn_shade_stage: the records filled into the context's own path buffers in the slots their pixels own,
a shuffled live queue, the renderer's own launcher) against the oracle's twin (orc.shade_stage: PathTracing::shade / ShadeMiss per record;
tests/test_shade_stage_cpu.py proves it is the oracle's loop).  Whole arrays, per set, in three steps:

  1. integers and decisions, no tolerance: flags, sampler dimension, membership in the next queue and in the shadow queue, light bits
  2. float fields whose vertex has no libm call between input and output, as bytes (NaN = NaN on both sides): `contrib` everywhere but
     at a miss under an environment map and at a toon first hit (a hit that emits nothing leaves it untouched; an emissive hit's MIS
     weight and a miss under a constant background are + - * / only); the next ray's origin and sh_o at EVERY vertex (ray_offset); the
     next direction, pdf and throughput behind a Specular or Refraction surface (reflect / refract and the roulette division are
     + - * / sqrt); sh_d, sh_dist and sh_c by light type and material (nee_exact)
  3. the remaining floats in the project's metric |got - want| / max(1, |want|), bounds from test_gpu_parity.py's material tables
     (BOUNDS below, written out per field)

Measured on an MI355X (docs/SHADE_STAGE.md has the table): no integer or decision differs in any set; every exact field is byte-equal;
the svgf flavour's AOV texels are byte-equal; every bounded field is inside its bound except `pdfb` at 0 to 7 vertices of a recorded frame
(7 of 16 401 in the atrium, 5 in atrium_ibl, 4 in sponza_disney, 0 to 3 elsewhere; worst 4.3e-2 at a Disney hit of the atrium) and one
throughput (atrium, svgf, 2.3e-3), which carry the named cause below -- the oracle itself moves further under one ulp of its input --
and are counted and reported.  The worst are kept as batches of their own (shade_vertices.FINDINGS).

The only vertices left out are those the margin rule of shade_vertices.py names, from the oracle's margins alone.  Flavours "plain" and
"svgf" (k_shade<true, MS> against svgf::Shade / ShadeMissAov, on sets chained through the svgf twin: shade_vertices.build_svgf); the
look-ahead, deferred-NEE, regenerated, five-wave and relaxed-math flavours are held to the plain kernel by tests/test_gpu_rr_lookahead.py,
test_gpu_nee_deferral.py, test_gpu_regen.py, test_gpu_config4.py and test_gpu_shade_math.py."""
import numpy as np
import pytest

import shade_vertices as V
from conftest import parity_record
from test_shade_stage_cpu import bits, sample_epilogue, LIGHT_MASK, STENCIL_BIT, F_TERMINATED

from aten_amd import layout as L

pytestmark = pytest.mark.gpu

INT_FIELDS = ("flags", "goes_on", "has_shadow", "dimension", "light_bits", "sh_c_w", "aov_written")
AOV_FIELDS = ("aov_nd", "aov_am", "aov_primary")        # flavour "svgf": the hit's normal, the fourth row of W2C times the hit point (the
                                                        # matrices are host arithmetic on both sides), a texel, ids: no libm call, as bytes
# The float bounds.  DIR and VAL are test_material_tables' (directions; pdf / bsdf values) for the sets of the base tier and
# test_material_tables_next_tier's for the others.  The rest are first-order sums over the factors of each field:
#   org, sh_o     ray_offset(p, n): p is exact, the offset follows the normal                                     -> DIR
#   dir, sh_d     a sampled / light direction behind a normalize                                                  -> DIR
#   sh_dist       length(pos - p): pos on the light, one sampled direction or point                               -> DIR
#   pdfb          the BSDF sample's pdf                                                                           -> VAL
#   throughput    thr_in * albedo * bsdf * c / pdf / rr:  bsdf (VAL) + pdf (VAL) + c = dot(n, dir) (2 DIR)        -> 2 VAL + 2 DIR
#   sh_c          thr_in * albedo * misW * bsdf * emit * G / ls.pdf / select:  misW (VAL: one pdf against another)
#                 + bsdf (VAL) + G = two cosines (4 DIR) + ls.pdf (its cosine and distance, 2 DIR)                -> 2 VAL + 6 DIR
#   contrib       contrib_in + thr * weight * emit at an environment-map miss (the weight is one pdf against another, the
#                 texel behind atan2 / acos) or the toon colour behind pow                                        -> VAL
BOUNDS = {}
for _tier, (_dir, _val) in {"base": (2e-5, 1e-3), "next": (5e-5, 2e-3)}.items():
    BOUNDS[_tier] = {"org": _dir, "dir": _dir, "sh_o": _dir, "sh_d": _dir, "sh_dist": _dir, "pdfb": _val,
                     "throughput": 2 * _val + 2 * _dir, "sh_c": 2 * _val + 6 * _dir, "contrib": _val}
EXACT_MATERIALS = (L.MTRL_SPECULAR, L.MTRL_REFRACTION)
# A NAMED CAUSE, the one test_material_tables documents: the lobe's condition number.  A microfacet pdf is D(h) cos / (4 |wo . h|); at a
# grazing half vector (a pdf of 600 where D is at most 32: wo . h = 0.013) or where a sharp lobe of a Disney sum is met off its own
# sample, a last-bit difference of a direction moves it by per cent.  That is MEASURED on the oracle, not assumed: such a vertex goes
# through the twin again with each component of its incoming direction one ulp up and one ulp down (ill_conditioning), and a value over
# its bound is accepted ONLY where
#   - its material evaluates a microfacet lobe (PEAKED_MATERIALS);
#   - the kernel's deviation is at most LIBM_ULPS = 2 times what ONE ulp of the input moves the oracle's own value (2 ulp: the libm
#     difference DESIGN section 4 states).  At the measured vertices one ulp moves the oracle's pdf by 1.7 % to 470 %; at their
#     neighbours by 1e-7, so the rule binds everywhere else;
#   - such vertices stay under NAMED_SHARE of the set's compared values (a tenth of what the margin rule may leave out).
# The throughput carries bsdf / pdf: where the two do not cancel (a Disney sum) it is held by the same rule.  Counted and reported.
PEAKED_MATERIALS = (L.MTRL_GGX, L.MTRL_BECKMAN, L.MTRL_DISNEY, L.MTRL_MICROFACET_REFRACTION, L.MTRL_RETROREFLECTIVE, L.MTRL_CARPAINT)
NAMED_SHARE = 1e-3
LIBM_ULPS = 2.0
NAMED_FIELDS = ("pdfb", "throughput")


# Which fields have NO libm call between input and output, from the list of libm calls in csrc/device/shading.hpp (diffuse_dir,
# ggx_sample_m, toon_specular_half, dis_gtr1, beckman_D, beckman_sample_m, velvet_*, retro_era, retro_rr_dir, direction_to_uv,
# uv_to_direction, ibl_texel_pdf, sample_light's sphere branch and its spot cone cosines):
#   org, sh_o          ray_offset(p, +-n): the hit point, the normal map, CarPaint's flake normal and ray_offset are + - * / sqrt and
#                      integer hashes                                                                           -> EVERY vertex
#   sh_d, sh_dist      sample_light of a point, spot or directional light and of an area light over triangles   -> by light type
#   sh_c               ... and the light's colour and the BSDF evaluation: not the spot light (cone cosines), and a surface whose
#                      evaluation is Lambert, Oren-Nayar or GGX (D, lambda and Schlick are + - * / sqrt)          -> light and material
NEE_EXACT_MATERIALS = (L.MTRL_DIFFUSE, L.MTRL_OREN_NAYAR, L.MTRL_GGX)


def nee_exact(vs, b):
    """(geometry exact, contribution exact) per vertex of the batch, from the light the oracle's shadow ray names."""
    lights, objs = vs.fs.arrays["lights"], vs.fs.arrays["objects"]
    if len(lights) == 0:
        z = np.zeros(len(b), bool)
        return z, z
    li = np.minimum((b.want["light_bits"] & LIGHT_MASK).astype(np.int64), len(lights) - 1)
    lt = lights["type"][li]
    oid = lights["arealight_objid"][li]
    poly = (lt == L.LIGHT_AREA) & (oid >= 0) & (objs["type"][np.maximum(oid, 0)] != L.OBJ_SPHERE)
    geo = np.isin(lt, (L.LIGHT_POINT, L.LIGHT_SPOT, L.LIGHT_DIRECTION)) | poly
    fallback = (b.rec["objid"] >= 0) & (b.mtype < 0)                # mtrlid < 0: the white Lambert material
    col = geo & (lt != L.LIGHT_SPOT) & (np.isin(b.mtype, NEE_EXACT_MATERIALS) | fallback) & ~b.has("toon_deep") & ~b.has("toon_first")
    return geo, col


def _ctx(vs, monkeypatch=None, waves=None):
    from aten_amd.renderer import PathTracing
    if monkeypatch is not None:
        if waves:
            monkeypatch.setenv("ATEN_AMD_SHADE_WAVES", str(waves))
        else:
            monkeypatch.delenv("ATEN_AMD_SHADE_WAVES", raising=False)
    r = PathTracing(0)
    try:
        r.UpdateSceneData(vs.fs)
        r.updateCamera(vs.cam)
        r.setRandom(vs.seeds)
        r.set_sampling_options(ibl_importance=vs.ibl_importance)
    except Exception:
        r.close()
        raise
    return r


def _run(r, vs, b, **kw):
    return r.shade_stage(b.rec, vs.w, vs.h, b.bounce, vs.depth, vs.rr, flavour=vs.flavour, **kw)


def _relerr(got, want):
    g = np.asarray(got, np.float64).reshape(len(got), -1); w = np.asarray(want, np.float64).reshape(len(want), -1)
    both_nan = np.isnan(g) & np.isnan(w)
    with np.errstate(invalid="ignore"):
        e = np.abs(g - w) / np.maximum(1.0, np.abs(w))
    e = np.where(both_nan, 0.0, e)
    return np.where(np.isnan(e), np.inf, e).max(axis=1) if len(e) else np.zeros(0)       # (NaN on one side only: infinitely far)


def _same_bytes(got, want):
    g = bits(got).reshape(len(got), -1); w = bits(want).reshape(len(want), -1)
    gn = np.isnan(np.asarray(got, np.float32)).reshape(g.shape); wn = np.isnan(np.asarray(want, np.float32)).reshape(w.shape)
    return np.all((g == w) | (gn & wn), axis=1)


def _describe(vs, b, i, field, got):
    from oracle import orc
    cats = [c for k, c in enumerate(orc.SHADE_CATEGORIES) if (int(b.cat[i]) >> k) & 1]
    return ("%s / %s bounce %d #%d pixel %d material %d [%s] margins %r: %s got %r, oracle %r"
            % (vs.name, b.label, b.bounce, i, int(b.rec["pixel"][i]), int(b.mtype[i]), " ".join(cats), b.margins[i].tolist(), field,
               got[field][i].tolist(), b.want[field][i].tolist()))


def compare(vs, b, got, stats):
    """The three steps on one batch; `stats` gathers per field {n, bit-equal, max error} for the report."""
    want, keep = b.want, b.compared
    # 1. integers and decisions
    for f in INT_FIELDS:
        bad = np.flatnonzero((got[f] != want[f]) & keep)
        assert len(bad) == 0, "%d of %d differ in %s; first: %s" % (len(bad), int(keep.sum()), f, _describe(vs, b, bad[0], f, got))
    on = keep & (want["goes_on"] != 0)
    sh = keep & (want["has_shadow"] != 0)
    miss = b.rec["objid"] < 0
    contrib_libm = (miss & vs.has_envmap) | b.has("toon_first")
    ray_exact = np.isin(b.mtype, EXACT_MATERIALS) & ~b.has("normal_map") & ~b.has("toon_deep")
    everywhere = np.ones(len(b), bool)
    for f in AOV_FIELDS:        # (zero on both sides where the bit of aov_written is clear, and everywhere in the plain flavour)
        bad = np.flatnonzero(keep & ~_same_bytes(got[f], want[f]))
        assert len(bad) == 0, "%d AOV texels differ in %s; first: %s" % (len(bad), f, _describe(vs, b, bad[0], f, got))
    nee_geo, nee_col = nee_exact(vs, b)
    plan = [("contrib", keep, ~contrib_libm), ("org", on, everywhere)] + [(f, on, ray_exact) for f in ("dir", "pdfb", "throughput")] \
        + [("sh_o", sh, everywhere), ("sh_d", sh, nee_geo), ("sh_dist", sh, nee_geo), ("sh_c", sh, nee_col)]
    for f, where, exact in plan:
        same = _same_bytes(got[f], want[f])
        err = _relerr(got[f], want[f])
        # 2. as bytes
        bad = np.flatnonzero(where & exact & ~same)
        assert len(bad) == 0, "%d vertices without a libm call differ in %s; first: %s" % (len(bad), f, _describe(vs, b, bad[0], f, got))
        # 3. bounded
        s = stats.setdefault(f, dict(n=0, bit_equal=0, max_err=0.0, over=0, got=[], want=[], first_over=None, exact=0))
        s["exact"] += int((where & exact).sum())
        s["n"] += int(where.sum()); s["bit_equal"] += int((where & same).sum())
        if where.any():
            s["max_err"] = max(s["max_err"], float(err[where].max()))
            s["got"].append(np.asarray(got[f][where], np.float32).reshape(int(where.sum()), -1))
            s["want"].append(np.asarray(want[f][where], np.float32).reshape(int(where.sum()), -1))
        over = where & (err > BOUNDS[vs.tier][f])
        if f in NAMED_FIELDS and over.any():
            cand = np.flatnonzero(over & np.isin(b.mtype, PEAKED_MATERIALS))
            named = np.zeros(len(b), bool)
            named[cand] = err[cand] <= LIBM_ULPS * V.ill_conditioning(vs, b, cand, f)
            s["named"] = s.get("named", 0) + int(named.sum())
            if named.any():
                s["named_max"] = max(s.get("named_max", 0.0), float(err[named].max()))
            over = over & ~named
        over = np.flatnonzero(over)
        s["over"] += len(over)
        if s["first_over"] is None and len(over):
            s["first_over"] = _describe(vs, b, over[0], f, got) + " (error %.3e)" % err[over[0]]


@pytest.mark.parametrize("name,flavour", [(n, "plain") for n in V.SETS] + [(n, "svgf") for n in V.SVGF_SETS])
def test_every_vertex_equals_the_twin(orc, cornell, sponza_disney, name, flavour):
    vs = (V.build if flavour == "plain" else V.build_svgf)(orc, name, cornell, sponza_disney)
    if flavour == "svgf":       # the chain reaches AOV writes at bounce 0, behind a Specular hit at bounce 1, and none deeper
        w = np.concatenate([b.want["aov_written"] for b in vs.batches])
        assert (w == 7).sum() >= V.FLOOR and (w == 0).sum() >= V.FLOOR
        assert name != "cornell" or (w == 3).sum() >= V.FLOOR
        name = name + "/svgf"
    r = _ctx(vs)
    stats = {}
    try:
        for b in vs.batches:
            compare(vs, b, _run(r, vs, b), stats)
    finally:
        r.close()
    failures = []
    for f, s in stats.items():
        bound = BOUNDS[vs.tier][f]
        print("shade stage %-14s %-10s n %7d  bit-equal %.4f  max error %.3e  bound %.1e  over %d  named (lobe's condition number) %d, max %.3e  asserted as bytes %d"
              % (name, f, s["n"], s["bit_equal"] / max(s["n"], 1), s["max_err"], bound, s["over"], s.get("named", 0), s.get("named_max", 0.0), s["exact"]))
        if s.get("named", 0) > NAMED_SHARE * s["n"]:
            failures.append("%s: %d of %d vertices claim the lobe's condition number" % (f, s["named"], s["n"]))
        if s["n"]:
            parity_record("shade_stage/%s/%s" % (name, f), np.concatenate(s["got"]), np.concatenate(s["want"]), tol=bound,
                          vertices=s["n"], bit_equal_vertices=s["bit_equal"], max_err_project_metric=s["max_err"], over_bound=s["over"],
                          named_lobe_condition_number=s.get("named", 0), named_max_err=s.get("named_max", 0.0), asserted_as_bytes=s["exact"])
        if s["over"]:
            failures.append("%s: %d of %d over %.1e (max %.3e); first: %s" % (f, s["over"], s["n"], bound, s["max_err"], s["first_over"]))
    assert not failures, "\n".join(failures)


COUNTS = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4099]


@pytest.mark.parametrize("flavour", ["plain", "svgf"])
@pytest.mark.parametrize("name", ["cornell", "atrium"])
def test_chunk_wave_and_block_edges(orc, cornell, sponza_disney, name, flavour):
    """Bounce 1's recorded vertices, repeated to 4099 on distinct pixels of a 96 x 96 frame: prefixes of every count, chunk_items 1 .. 4
    and the plan's, queue orders hits first / misses first / alternating / shuffled -- each result byte-equal to the same record's in
    the full run.  The hits-first LDS permutation and block_append2 neither drop, duplicate nor cross-wire a slot."""
    vs = V.build(orc, name, cornell, sponza_disney)
    if flavour == "svgf":
        vs = V.build_svgf(orc, name, cornell, sponza_disney)
    b = [x for x in vs.batches if x.bounce == 1 and x.label in ("recorded", "chained")][0]
    w = h = 96
    rng = np.random.default_rng(3)
    base = np.resize(b.rec, COUNTS[-1]).copy()
    base["pixel"] = rng.permutation(w * h)[:len(base)]
    is_hit = base["objid"] >= 0
    assert 0.02 < is_hit.mean() < 0.98
    big = V.VertexSet(name, vs.fs, orc.create_camera(vs.cam_dict["pos"], vs.cam_dict["at"], vs.cam_dict["vfov"], w, h), orc.init_sampler(w, h, 0),
                      w, h, vs.depth, vs.rr, vs.ibl_importance, vs.tier)
    r = _ctx(big)
    try:
        full = r.shade_stage(base, w, h, 1, vs.depth, vs.rr, flavour=flavour)
        assert flavour == "plain" or name != "cornell" or (full["aov_written"] == 3).any()      # (AOVs behind the Cornell box's mirror)
        assert full["goes_on"].any() and full["has_shadow"].any() and not full["goes_on"].all()
        for n in COUNTS:
            hits, misses = np.flatnonzero(is_hit[:n]), np.flatnonzero(~is_hit[:n])
            k = min(len(hits), len(misses))
            alt = np.concatenate([np.stack([hits[:k], misses[:k]], 1).ravel(), hits[k:], misses[k:]])
            orders = {"hits first": (np.concatenate([hits, misses]), "given"), "misses first": (np.concatenate([misses, hits]), "given"),
                      "alternating": (alt, "given"), "shuffled": (np.arange(n), "shuffled")}
            for items in (1, 2, 3, 4, 0):
                for label, (perm, order) in orders.items():
                    got = r.shade_stage(base[perm], w, h, 1, vs.depth, vs.rr, chunk_items=items, queue_order=order, flavour=flavour)
                    assert got.tobytes() == full[perm].tobytes(), "%s: n %d, chunk_items %d, %s" % (name, n, items, label)
    finally:
        r.close()


@pytest.mark.parametrize("name", ["cornell", "sponza_disney", "extra", "carpaint", "toon"])
def test_four_and_five_waves(monkeypatch, orc, cornell, sponza_disney, name):
    """ATEN_AMD_SHADE_WAVES = 4 and 5 (k_shade_wn where the material set has it) give the bytes of the context's own choice."""
    vs = V.build(orc, name, cornell, sponza_disney)
    batches = [x for x in vs.batches if x.label == "recorded"]
    results = {}
    for waves in (None, 4, 5):
        r = _ctx(vs, monkeypatch, waves)
        try:
            results[waves] = [_run(r, vs, b).tobytes() for b in batches]
        finally:
            r.close()
    assert results[4] == results[None] and results[5] == results[None]


def test_the_probe_is_the_frame(gpu, orc, cornell):
    """generate_paths -> trace_closest -> shade_stage -> trace_shadow per bounce on the GPU, the sample epilogue in NumPy: atn_render's film."""
    fs, cam = cornell
    w = h = 64
    depth, rr = 5, 3
    c = orc.create_camera(cam["pos"], cam["at"], cam["vfov"], w, h)
    gpu.UpdateSceneData(fs); gpu.updateCamera(c); gpu.initSampler(w, h, 0); gpu.setScreenShard(0, 1); gpu.reset()
    film = gpu.render(w, h, depth, rr, frame=0, progressive=False)
    rays = gpu.generate_paths(w, h, 0, 0)
    rec = np.zeros(w * h, L.SHADE_VERTEX)
    rec["org"] = rays["org"]; rec["dir"] = rays["dir"]; rec["pdfb"] = 1.0; rec["throughput"] = 1.0
    rec["dimension"] = 2                    # GeneratePath drew the pixel jitter
    rec["pixel"] = np.arange(w * h)
    final = np.zeros((w * h, 3), np.float32)
    for bounce in range(depth):
        ray = np.zeros(len(rec), L.RAY); ray["org"] = rec["org"]; ray["dir"] = rec["dir"]
        hit = gpu.trace_closest(ray)
        for f in ("objid", "a", "b", "tri_id"):
            rec[f] = hit[f]
        rec["objid"][hit["objid"] < 0] = -1
        res = gpu.shade_stage(rec, w, h, bounce, depth, rr)
        total = res["contrib"].copy()
        s = np.flatnonzero(res["has_shadow"] != 0)
        if len(s):
            vis = gpu.trace_shadow(res["sh_o"][s], res["sh_d"][s], res["sh_dist"][s], (res["light_bits"][s] & LIGHT_MASK).astype(np.int32),
                                   (res["light_bits"][s] & STENCIL_BIT) != 0).astype(bool)
            total[s[vis]] = (total[s[vis]] + res["sh_c"][s[vis]]).astype(np.float32)
        on = res["goes_on"] != 0
        final[rec["pixel"][~on]] = total[~on]
        nxt = np.zeros(int(on.sum()), L.SHADE_VERTEX)
        for f in ("org", "dir", "pdfb", "throughput", "dimension", "flags"):
            nxt[f] = res[f][on]
        nxt["contrib"] = total[on]; nxt["pixel"] = rec["pixel"][on]
        rec = nxt
        if not len(rec):
            break
    assert len(rec) == 0
    want = sample_epilogue(final.reshape(h, w, 3))
    assert np.array_equal(bits(want), bits(film))


def test_probe_errors(gpu, orc, cornell):
    from aten_amd.renderer import PathTracing, AtenAmdError
    vs = V.build(orc, "cornell", cornell)
    b = vs.batches[1]
    rec = b.rec[:8].copy()
    r = PathTracing(0)
    try:
        with pytest.raises(AtenAmdError, match="status -4"):           # no scene
            r.shade_stage(rec, vs.w, vs.h, 1, vs.depth, vs.rr)
        r.UpdateSceneData(vs.fs); r.updateCamera(vs.cam); r.setRandom(vs.seeds)
        assert len(r.shade_stage(rec[:0], vs.w, vs.h, 1, vs.depth, vs.rr)) == 0       # n = 0 returns empty
        ok = r.shade_stage(rec, vs.w, vs.h, 1, vs.depth, vs.rr)
        call = L.shade_call(vs.w, vs.h, 1, vs.depth, vs.rr)
        out = np.zeros(len(rec), L.SHADE_RESULT)
        assert r._l.atn_shade_stage(r._ctx, None, rec.ctypes.data, len(rec), out.ctypes.data) == -1         # null pointers
        assert r._l.atn_shade_stage(r._ctx, call.ctypes.data, None, len(rec), out.ctypes.data) == -1
        assert r._l.atn_shade_stage(r._ctx, call.ctypes.data, rec.ctypes.data, len(rec), None) == -1
        dup = rec.copy(); dup["pixel"][3] = dup["pixel"][5]
        with pytest.raises(AtenAmdError, match="status -1"):           # duplicate pixels
            r.shade_stage(dup, vs.w, vs.h, 1, vs.depth, vs.rr)
        for pixel in (vs.w * vs.h, -1):                                 # a pixel outside the frame
            bad = rec.copy(); bad["pixel"][2] = pixel
            with pytest.raises(AtenAmdError, match="status -1"):
                r.shade_stage(bad, vs.w, vs.h, 1, vs.depth, vs.rr)
        for bounce in (vs.depth, vs.depth + 3, -1):                     # a bounce at or beyond max_depth
            with pytest.raises(AtenAmdError, match="status -1"):
                r.shade_stage(rec, vs.w, vs.h, bounce, vs.depth, vs.rr)
        with pytest.raises(ValueError):                                 # an unknown flavour (by name, and by number below)
            r.shade_stage(rec, vs.w, vs.h, 1, vs.depth, vs.rr, flavour="lookahead")
        # "svgf" on a context that never rendered an SVGF frame: the entry allocates its own three AOV planes, so it is served -- and
        # leaves the plain flavour's result of the same records alone
        sv = r.shade_stage(rec, vs.w, vs.h, 1, vs.depth, vs.rr, flavour="svgf")
        assert np.array_equal(sv["goes_on"], ok["goes_on"]) and not ok["aov_written"].any()
        for field, value in (("flavour", 2), ("flavour", -1), ("chunk_items", 5), ("chunk_items", -1), ("queue_order", 2)):
            c2 = call.copy(); c2[field] = value
            assert r._l.atn_shade_stage(r._ctx, c2.ctypes.data, rec.ctypes.data, len(rec), out.ctypes.data) == -1, (field, value)
        term = rec.copy(); term["flags"][0] |= F_TERMINATED
        with pytest.raises(AtenAmdError, match="status -1"):           # a terminated record is not in a live queue
            r.shade_stage(term, vs.w, vs.h, 1, vs.depth, vs.rr)
        hit = int(np.flatnonzero(rec["objid"] >= 0)[0])
        for field, value in (("tri_id", 1 << 30), ("objid", 1 << 20), ("a", np.nan)):
            bad = rec.copy(); bad[field][hit] = value
            with pytest.raises(AtenAmdError, match="status -1"):       # a hit record outside the scene
                r.shade_stage(bad, vs.w, vs.h, 1, vs.depth, vs.rr)
        assert r.shade_stage(rec, vs.w, vs.h, 1, vs.depth, vs.rr).tobytes() == ok.tobytes()       # the context stays usable
    finally:
        r.close()
