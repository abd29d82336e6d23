"""Analytic spheres without a GPU (docs/SPHERES.md): the CPU twin (tests/sphere_oracle.py) against the oracle where no sphere leaf
exists, the host upload's sphere records (a stand-alone program, also under AddressSanitizer + UBSan), and the twin's walk against the
float64 classifier of tests/sphere_cases.py."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import brute_force as B
import sphere_cases as SC
import sphere_oracle as SO
from conftest import ROOT, make_camera

SETS = ["sphere_cornell", "spheres3", "sphere_only", "spheres_sponza"]
N_PER_SET = 1000        # (x 4.5: aimed, random, surface, inside, and the straddle set twice a quarter)


def test_abi_symbols_and_header():
    from aten_amd._lib import SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "aten_amd.h")).read()
    for s in ("atn_set_sphere_intersection", "atn_sphere_leaves", "atn_mgpu_set_sphere_intersection"):
        assert s in SYMBOLS and ("int %s(" % s) in hdr, s
    from aten_amd.renderer import PathTracing, MultiGpuPathTracing as MultiGpu
    assert hasattr(PathTracing, "set_sphere_intersection") and hasattr(PathTracing, "sphere_leaves") and hasattr(MultiGpu, "set_sphere_intersection")


def test_twin_is_the_oracle_without_sphere_leaves(orc, cornell):
    """Closure: on a scene without sphere leaves the twin's frames, hits and verdicts are the oracle's, byte for byte."""
    fs, cam = cornell
    W, H = 64, 48
    c = make_camera(orc, cam, W, H)
    seeds = orc.init_sampler(W, H, 0)
    fa = np.zeros((H, W, 4), np.float32); fb = np.zeros((H, W, 4), np.float32)
    for frame in range(2):
        orc.render(fs, c, seeds, W, H, 5, 3, frame=frame, film=fa)
        SO.render(fs, c, seeds, W, H, 5, 3, frame=frame, film=fb)
        assert fa.tobytes() == fb.tobytes(), "frame %d" % frame
    rays = orc.generate_paths(c, seeds, W, H, 0, 0)
    assert SO.trace_closest(fs, rays).tobytes() == orc.trace_closest(fs, rays)[0].tobytes()


def _build_upload_test(tmp_path, name, extra):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / name)
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O1", "-w", "-I", os.path.join(ROOT, "include")] + extra
                          + [os.path.join(ROOT, "tests", "cxx", "sphere_upload_test.cpp"), "-o", exe])
    return exe


def test_upload_host_logic(tmp_path):
    """tests/cxx/sphere_upload_test.cpp: mode 0 is the upload as it was, mode 1 differs in the sphere record and the links that name it,
    every refusal fires."""
    out = subprocess.run([_build_upload_test(tmp_path, "sphere_upload_test", [])], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr


def test_upload_host_logic_sanitized(tmp_path):
    """The same stand-alone program with its host code under AddressSanitizer + UBSan."""
    exe = _build_upload_test(tmp_path, "sphere_upload_test_san", ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-g"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=180, env=env)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok") and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stdout + out.stderr


_truth = {}


def truth(name):
    """(scene, rays, float64 answer, twin's INTERSECTION) per scene, computed once and shared (the GPU tests read it too)."""
    if name not in _truth:
        fs, _ = SC.scene(name)
        rays = SC.ray_sets(fs, seed=20 + SETS.index(name), n=N_PER_SET)
        ans = SC.classify(fs, rays.org, rays.dir, t_max=rays.t_max)
        twin = B.trace(lambda rec, t_min, t_max: SO.trace_closest(fs, rec, t_min, t_max), rays)
        _truth[name] = (fs, rays, ans, twin)
    return _truth[name]


# The outcome whose share of a set is held to brute_force.FLOOR on both sides: in the sets aimed at spheres "a sphere is reported", in
# the sets with a t_max "a hit within t_max" (a report beyond it reads as a miss: SC.canonical).  One set has one outcome whatever rays
# it holds, by the isClose rule the set exists to hold: born on the only sphere of sphere_only, no ray can hit anything.
ONE_OUTCOME = {("sphere_only", "surface"): 0.0}


def check_against_float64(name, rays, ans, got, what):
    """The rules of tests/brute_force.py carried over: decided rays match exactly (object, tri = -1 for a sphere, hit or miss), the
    others report a candidate, a report beyond t_max is a real hit; per set at most 3 % undecided and each outcome at least 5 %;
    'surface' rays never report their own sphere.  Returns the largest |t - t64| / max(t, 1e-3 diagonal) over the decided sphere hits."""
    fs, _ = SC.scene(name)
    objid, tri, beyond_ok = SC.canonical(fs, rays, got, ans)
    ok = SC.in_candidates(ans, objid, tri) & beyond_ok
    bad = np.flatnonzero(~ok)
    assert len(bad) == 0, "%s %s: %d rays off, first %s: got (%d, %d) t %r t_max %r want (%d, %d) decided %s" % (
        name, what, len(bad), rays.set[bad[0]], got["objid"][bad[0]], got["tri_id"][bad[0]], float(got["t"][bad[0]]), float(rays.t_max[bad[0]]),
        ans.objid[bad[0]], ans.tri_id[bad[0]], ans.decided[bad[0]])
    for s in np.unique(rays.set):
        m = rays.set == s
        und = 1.0 - ans.decided[m].mean()
        assert und <= B.UNDECIDED_CAP, "%s %s: %.3f of set %s undecided" % (name, what, und, s)
        share = float(((objid[m] >= 0) & (tri[m] < 0)).mean()) if s in ("aimed", "random") else float((objid[m] >= 0).mean())
        if (name, s) in ONE_OUTCOME:
            assert share == ONE_OUTCOME[(name, s)], "%s %s: set %s share %.3f" % (name, what, s, share)
        else:
            assert B.FLOOR <= share <= 1 - B.FLOOR, "%s %s: set %s share %.3f" % (name, what, s, share)
    sm = rays.set == "surface"
    own = SC.surface_owner(fs, rays.take(np.flatnonzero(sm)))
    g = got[sm]
    assert not np.any((g["tri_id"] < 0) & (g["objid"] == own)), "%s %s: a ray born on a sphere reports that sphere" % (name, what)
    d = ans.decided & ans.hit & (objid == ans.objid) & (tri == ans.tri_id)
    diag = SC.diagonal(fs)
    rel = np.abs(got["t"][d].astype(np.float64) - ans.t[d]) / np.maximum(ans.t[d], 1e-3 * diag)
    sph = tri[d] < 0
    return float(rel[sph].max()) if sph.any() else 0.0


@pytest.mark.parametrize("name", SETS)
def test_twin_against_float64(name):
    fs, rays, ans, twin = truth(name)
    worst = check_against_float64(name, rays, ans, twin, "twin")
    # float32 sphere::hit against float64: b and sqrt(D4) carry ~1e-7 relative error each, t1 = b - sqrt(D4) cancels by at most the
    # ratio origin distance / t -- the aimed set starts within 4 r + 0.05 diagonal of the centre
    assert worst <= 1e-4, worst
    if os.environ.get("ATEN_BRUTE_FORCE_RECORD") == "1":
        path = os.path.join(ROOT, "profiles", "parity_spheres.jsonl")
        with open(path, "a") as f:
            f.write(json.dumps(dict(case=name, rays=len(rays), decided=float(ans.decided.mean()), sphere_hits=int((twin["tri_id"] < 0)[twin["objid"] >= 0].sum()),
                                    max_rel_t_err_sphere_hits=worst)) + "\n")


@pytest.mark.parametrize("name", SETS)
def test_twin_shadow_verdicts_against_float64(orc, name):
    """Shadow queries towards every light of the scene: where float64 is decided, the twin's verdict is its verdict."""
    fs, _ = SC.scene(name)
    n_dec = 0
    for li in SC.shadow_lights(fs):
        o, d, dist = SC.shadow_set(fs, li, seed=70 + li)
        want, decided = SC.shadow_truth(fs, li, o, d, dist)
        got = SO.shadow_visible(fs, orc.shadow_queries(o, d, dist, li)).astype(bool)
        assert np.array_equal(got[decided], want[decided]), "%s light %d: %d verdicts differ" % (name, li, int((got[decided] != want[decided]).sum()))
        assert decided.mean() >= 1 - B.UNDECIDED_CAP, (name, li, decided.mean())
        assert B.FLOOR <= want[decided].mean() <= 1 - B.FLOOR, (name, li, want[decided].mean())
        n_dec += int(decided.sum())
    assert n_dec > 0
