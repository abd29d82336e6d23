"""ctypes binding of tests/cxx/taa_oracle.cpp, the CPU restatement of the reference's TAA and gamma shaders (docs/TAA.md).  TEST
INFRASTRUCTURE ONLY: compiled with g++ into a temporary directory once per session, loaded by tests; the product never imports it."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cxx", "taa_oracle.cpp")
_lib = None
_dir = None


def lib():
    global _lib, _dir
    if _lib is None:
        _dir = tempfile.mkdtemp(prefix="taa_oracle_")
        so = os.path.join(_dir, "libtaa_oracle.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-o", so, SRC])
        l = C.CDLL(so)
        vp, f, i = C.c_void_p, C.c_float, C.c_int32
        l.orc_taa_resolve.argtypes = [i, i, vp, vp, vp, i, f, vp, vp, vp, vp, vp]
        l.orc_taa_resolve.restype = None
        l.orc_taa_sample_color.argtypes = [vp, vp]; l.orc_taa_sample_color.restype = None
        l.orc_taa_clip.argtypes = [vp, vp, vp, vp]; l.orc_taa_clip.restype = None
        l.orc_taa_box.argtypes = [i, i, vp, i, i, vp, vp]; l.orc_taa_box.restype = None
        l.orc_taa_tap.argtypes = [i, i, vp, i, i, vp, vp, vp]; l.orc_taa_tap.restype = None
        l.orc_taa_unorm8.argtypes = [vp, i, vp]; l.orc_taa_unorm8.restype = None
        _lib = l
    return _lib


def _p(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def _plane(a):
    a = np.ascontiguousarray(a, np.float32)
    assert a.ndim == 3 and a.shape[2] == 4
    return a


def resolve(cur, hist, motion, enable=True, gamma=2.2, extras=False):
    """One frame over planes [h, w, 4] (row 0 = bottom); hist None = no history (the first-frame rule).  Returns (out, gamma float,
    rgba8 uint32 [h, w]) and with extras=True also (exp arguments, weights), both [h, w, 9] with NaN for taps not taken."""
    cur, motion = _plane(cur), _plane(motion)
    hist = _plane(hist) if hist is not None else None
    h, w = cur.shape[:2]
    assert motion.shape == cur.shape and (hist is None or hist.shape == cur.shape)
    out = np.zeros_like(cur)
    gf = np.zeros_like(cur)
    g8 = np.zeros((h, w), np.uint32)
    ea = np.zeros((h, w, 9), np.float32) if extras else None
    ws = np.zeros((h, w, 9), np.float32) if extras else None
    lib().orc_taa_resolve(w, h, _p(cur), _p(hist), _p(motion), int(bool(enable)), float(gamma), _p(out), _p(gf), _p(g8), _p(ea), _p(ws))
    return (out, gf, g8, ea, ws) if extras else (out, gf, g8)


def sample_color(c):
    c = np.ascontiguousarray(c, np.float32)
    out = np.zeros(4, np.float32)
    lib().orc_taa_sample_color(_p(c), _p(out))
    return out


def clip(mn, mx, q):
    mn, mx, q = (np.ascontiguousarray(v, np.float32) for v in (mn, mx, q))
    out = np.zeros(3, np.float32)
    lib().orc_taa_clip(_p(mn), _p(mx), _p(q), _p(out))
    return out


def box(cur, ix, iy):
    cur = _plane(cur)
    mn, mx = np.zeros(4, np.float32), np.zeros(4, np.float32)
    lib().orc_taa_box(cur.shape[1], cur.shape[0], _p(cur), int(ix), int(iy), _p(mn), _p(mx))
    return mn, mx


def tap(hist, ix, iy, md):
    """The raw bilinear history fetch of pixel (ix, iy)'s centre for the motion/depth texel md, and the uv it was made at."""
    hist = _plane(hist)
    md = np.ascontiguousarray(md, np.float32)
    out, uv = np.zeros(4, np.float32), np.zeros(2, np.float32)
    lib().orc_taa_tap(hist.shape[1], hist.shape[0], _p(hist), int(ix), int(iy), _p(md), _p(out), _p(uv))
    return out, uv


def unorm8(g):
    g = np.ascontiguousarray(g, np.float32).ravel()
    out = np.zeros(g.size, np.uint32)
    lib().orc_taa_unorm8(_p(g), g.size, _p(out))
    return out


GPU_CASES = [(1, 1, 101), (13, 7, 102), (40, 67, 103)]     # (w, h, seed) of tests/test_gpu_taa.py: every tap clamps to the pixel; less
#                                                            than one 8 x 32 tile, ragged; several tiles on both axes, both sizes ragged
GAMMA = 2.2


def run_twin(frames, hist=None, gamma=GAMMA):
    """Consecutive frames through the twin, each one's output the next one's history (hist None: the first frame has none).
    Returns a list of dicts out, gamma, rgba8, exp_args, weights."""
    res = []
    for col, mot in frames:
        out, gf, g8, ea, ws = resolve(col, hist, mot, gamma=gamma, extras=True)
        res.append(dict(out=out, gamma=gf, rgba8=g8, exp_args=ea, weights=ws))
        hist = out
    return res


def make_inputs(w, h, seed, moving=True):
    """The planes of tests/test_gpu_taa.py: seeded HDR colour in [0, 8] with zeros, a few 1e8 pixels and saturated red / green pairs
    planted; motion that is zero, sub-texel, whole-texel, of magnitude 1.5 and pointing out of the frame on all four sides; depth < 0
    on about 10 % of the pixels, isolated ones and a whole row; in frames of 8 x 8 and more a 3 x 3 block of 1e8 that stays in place (inf, then NaN).  moving=False: the same colours and depths with all motion zero.
    Returns three frames' (colour, motion) and the history uploaded before the first of them."""
    rng = np.random.default_rng(seed)
    n = w * h
    frames = []
    for f in range(3):
        col = (rng.random((h, w, 4), np.float32) * np.float32(8.0)).astype(np.float32)
        col[..., 3] = rng.random((h, w), np.float32)
        flat = col.reshape(n, 4)
        k = max(1, n // 16)
        flat[rng.choice(n, k, replace=False), :3] = 0.0
        flat[rng.choice(n, max(1, n // 64), replace=False), :3] = np.float32(1e8)
        for i in rng.choice(n, k, replace=False):      # saturated red next to saturated green: the chroma limiter
            flat[i, :3] = (8.0, 0.0, 0.0)
            flat[(i + 1) % n, :3] = (0.0, 8.0, 0.0)
        mot = np.zeros((h, w, 4), np.float32)
        mot[..., 2] = rng.random((h, w), np.float32) * 10 + np.float32(0.1)
        mot[..., 3] = 1.0
        if moving:
            kind = rng.integers(0, 8, (h, w))
            sub = (rng.random((h, w, 2), np.float32) - np.float32(0.5)) * np.float32(1.5) / np.array([w, h], np.float32)
            whole = rng.integers(-2, 3, (h, w, 2)).astype(np.float32) / np.array([w, h], np.float32)
            ang = rng.random((h, w), np.float32) * np.float32(6.2831853)
            big = np.stack([np.cos(ang), np.sin(ang)], -1).astype(np.float32) * np.float32(1.5)
            side = np.array([[-0.75, 0.0], [0.75, 0.0], [0.0, -0.75], [0.0, 0.75]], np.float32)[rng.integers(0, 4, (h, w))]
            mv = np.where((kind == 1)[..., None] | (kind == 2)[..., None], sub, 0.0)
            mv = np.where((kind == 3)[..., None] | (kind == 4)[..., None], whole, mv)
            mv = np.where((kind == 5)[..., None], big, mv)
            mv = np.where((kind >= 6)[..., None], side, mv)
            mot[..., :2] = mv.astype(np.float32)
        miss = rng.random((h, w)) < 0.08
        if h > 2:
            miss[h // 2, :] = True         # a whole row
        mot[miss, 2] = -1.0
        if w >= 8 and h >= 8:
            # a 3 x 3 block of 1e8 that stays where it is: its centre resolves to +inf in the second frame and to NaN in the third
            col[2:5, 3:6, :3] = np.float32(1e8)
            mot[2:5, 3:6] = (0.0, 0.0, 1.0, 1.0)
        frames.append((col, mot))
    hist = (rng.random((h, w, 4), np.float32) * np.float32(8.0)).astype(np.float32)
    return frames, hist


def excluded(out, weights):
    """Pixels [h, w] whose finite components the moving-plane comparison may leave out: they went through the resolve (some tap counted)
    and unmap divided by 1 - lum < 2^-10 there.  out = rgb / (1 - lum) with lum = Y(rgb), so 1 - lum = 1 / (1 + Y(out))."""
    with np.errstate(all="ignore"):
        wsum = np.nansum(weights.astype(np.float64), axis=-1)
        resolved = (wsum > 0) & ~np.all(np.isnan(weights), axis=-1)
        o = out.astype(np.float64)
        y = o[..., 0] / 4 + o[..., 1] / 2 + o[..., 2] / 4
        d = 1.0 / (1.0 + y)
        return resolved & ~(d >= 2.0 ** -10)
