"""The per-ray gate of the shadow job: every query's visible / not-visible verdict from the PRODUCTION shadow kernels (PathTracing.trace_shadow
-> atn_trace_shadow: path buffers filled as the shade stage leaves them, a shuffled queue over every second slot, the renderers' own
launchers) equals the oracle's HitTestToTargetLight (orc.shadow_visible), whole arrays, no tolerance, nothing excluded.

Ray sets and scenes: tests/shadow_rays.py (categories A .. E; tests/test_shadow_oracle_cpu.py holds the same sets against independent
restatements on the CPU).  Every scene runs on the walk its tree calls for and under ATEN_AMD_TRACE=r (the lane-refilling walk); the
Cornell box also with ATEN_AMD_LDS_NODES=0 (the plain walk over global memory): the three copies of the stop rule and of the twin-root
selection in device/traverse.hpp.  Flavours: "fused" and "counted" for every category, "deferred" and "regen" for A and D."""
import numpy as np
import pytest

import shadow_rays as S

pytestmark = pytest.mark.gpu

WALKS = ["own", "refill"]


def _ctx(monkeypatch, walk, fs, plain=True, **upload):
    from aten_amd.renderer import PathTracing
    if walk == "refill":
        monkeypatch.setenv("ATEN_AMD_TRACE", "r")
    else:
        monkeypatch.delenv("ATEN_AMD_TRACE", raising=False)
    if walk == "global":
        monkeypatch.setenv("ATEN_AMD_LDS_NODES", "0")
    else:
        monkeypatch.delenv("ATEN_AMD_LDS_NODES", raising=False)
    if plain:
        monkeypatch.delenv("ATEN_AMD_SHADOW_PLAIN", raising=False)
    else:
        monkeypatch.setenv("ATEN_AMD_SHADOW_PLAIN", "0")
    r = PathTracing(0)
    try:
        if upload:
            r.set_upload_options(**upload)
        r.UpdateSceneData(fs)
    except Exception:
        r.close()
        raise
    return r


def _flavours(rs):
    """(flavour, the rays it runs on): fused and counted on everything, deferred and regen on categories A and D."""
    ad = np.flatnonzero(np.isin(np.array([c[0] for c in rs.cat]), ["A", "D"]))
    out = [("fused", None), ("counted", None)]
    if len(ad):
        out += [("deferred", ad), ("regen", ad)]
    return out


def _compare(r, rs, want, what):
    for flavour, idx in _flavours(rs):
        sub, w = (rs, want) if idx is None else (rs.take(idx), want[idx])
        final = (np.arange(len(sub)) % 3 == 1) if flavour == "regen" else None
        got = r.trace_shadow(sub.org, sub.dir, sub.dist, sub.light, sub.stencil, flavour=flavour, final=final)
        assert np.array_equal(got, w), "%s, %s:\n%s" % (what, flavour, S.mismatch_report(sub, got, w))


def _walks(name):
    return WALKS + (["global"] if name == "cornell" else [])


@pytest.mark.parametrize("name,walk", [(n, w) for n in S.CASES for w in _walks(n)])
def test_every_verdict_equals_the_oracle(monkeypatch, orc, cornell, name, walk):
    fs, _, rs, want = S.case(orc, name, cornell)
    S.check_floor(rs, want, name)
    cats = S.CASES[name][1]
    # C: with the planar-light certificate and without; a scene under infinite lights only: with the plain job and with the generic one
    variants = [dict()]
    if "C" in cats:
        variants = [dict(planar_lights=1), dict(planar_lights=0)]
    directional = "directional" in name
    for v in variants:
        for plain in ((True, False) if directional else (True,)):
            r = _ctx(monkeypatch, walk, fs, plain=plain, **v)
            try:
                if "C" in cats:
                    assert r.planar_area_lights() == v["planar_lights"]
                _compare(r, rs, want, "%s, %s walk, %r, plain job %s" % (name, walk, v, plain))
            finally:
                r.close()


@pytest.mark.parametrize("walk", WALKS)
@pytest.mark.parametrize("name", ["cornell", "mixed", "sponza", "atrium"])
def test_query_counts_around_the_wave_the_chunk_and_the_block(monkeypatch, orc, cornell, name, walk):
    """Category E's rays in prefixes of 1, 63, 64, 65, 1023, 1024, 1025 and 4099 queries (repeated to that length where the set is shorter)."""
    fs, _, rs, want = S.case(orc, name, cornell)
    e = np.flatnonzero(np.array([c[0] for c in rs.cat]) == "E")
    r = _ctx(monkeypatch, walk, fs)
    try:
        for n in S.E_SIZES:
            idx = np.resize(e, n)
            sub, w = rs.take(idx), want[idx]
            for flavour in ("fused", "counted"):
                got = r.trace_shadow(sub.org, sub.dir, sub.dist, sub.light, sub.stencil, flavour=flavour)
                assert np.array_equal(got, w), "%s, %s walk, n = %d, %s:\n%s" % (name, walk, n, flavour, S.mismatch_report(sub, got, w))
    finally:
        r.close()


# F: (anyhit_twin, anyhit_twin_dirs, node_layout)
UPLOADS = [(1, 8, 1), (1, 1, 1), (0, 8, 1), (2, 8, 0), (2, 1, 0), (0, 8, 0)]


@pytest.mark.parametrize("walk", WALKS)
@pytest.mark.parametrize("name", ["sponza", "atrium"])
def test_upload_options_do_not_move_a_verdict(monkeypatch, orc, name, walk):
    fs, _, rs, want = S.case(orc, name)
    for twin, dirs, layout in UPLOADS:
        r = _ctx(monkeypatch, walk, fs, anyhit_twin=twin, anyhit_twin_dirs=dirs, node_layout=layout)
        try:
            # (mode 1 builds twins only where the surface-area model expects them to pay: none in the small atrium)
            if twin != 1:
                assert (r.anyhit_twins() > 0) == (twin == 2), (twin, dirs, layout, r.anyhit_twins())
            _compare(r, rs, want, "%s, %s walk, twins %d, twin dirs %d, node layout %d" % (name, walk, twin, dirs, layout))
        finally:
            r.close()


def test_probe_errors(gpu, orc, cornell):
    from aten_amd.renderer import PathTracing, AtenAmdError
    from aten_amd.scene.builder import SceneBuilder
    from aten_amd import layout as L
    fs, _ = cornell
    o, d = np.zeros((2, 3), np.float32), np.tile(np.array([0, 1, 0], np.float32), (2, 1))
    r = PathTracing(0)
    try:
        with pytest.raises(AtenAmdError, match="status -4"):           # no scene
            r.trace_shadow(o, d, 1.0, 0)
        r.UpdateSceneData(fs)
        assert len(r.trace_shadow(o[:0], d[:0], np.zeros(0, np.float32), np.zeros(0, np.int32))) == 0
        for bad in (1, -1):                                             # a light index outside the scene's lights
            with pytest.raises(AtenAmdError, match="status -1"):
                r.trace_shadow(o, d, 1.0, bad)
        with pytest.raises(ValueError):
            r.trace_shadow(o, d, 1.0, 0, flavour="eager")
        q = np.zeros(2, L.SHADOW_QUERY)
        out = np.zeros(2, np.uint8)
        assert r._l.atn_trace_shadow(r._ctx, q.ctypes.data, 2, 4, out.ctypes.data) == -1       # an unknown flavour
        assert r._l.atn_trace_shadow(r._ctx, None, 2, 0, out.ctypes.data) == -1                # null pointers
        assert r._l.atn_trace_shadow(r._ctx, q.ctypes.data, 2, 0, None) == -1
        # a scene without lights
        b = SceneBuilder()
        m = b.add_material("white", L.MTRL_DIFFUSE, (0.7, 0.7, 0.7))
        b.create_instance(b.add_mesh("floor", np.array([[-1, 0, -1], [1, 0, -1], [1, 0, 1], [-1, 0, 1]], np.float32), [[0, 2, 1], [0, 3, 2]], m))
        r.UpdateSceneData(b.build())
        with pytest.raises(AtenAmdError, match="status -5"):
            r.trace_shadow(o, d, 1.0, 0)
    finally:
        r.close()
