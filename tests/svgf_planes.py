"""Synthetic SVGF input planes for the edge tests (tests/test_gpu_svgf_edges.py, tests/test_oracle_svgf_cpu.py).  TEST INFRASTRUCTURE
ONLY: a plain helper module, deterministic from (w, h, frame, seed); no scene, no renderer.

What the planes are made of, and why:
  mesh ids    up to six regions cut by two stair-stepped columns and one row whose positions are odd and no multiple of 8, so that
              no boundary lines up with a tile (8), a pixel group (2 * 2^i) or a block row (32); every frame edge has a region on it
  background  albedo_meshid.w = -1 and normal_depth = (0, 0, 0, -1) (FillBasicAOVsIfHitMiss): single pixels, a run along the top row,
              a run along the right column and the bottom-left corner
  normals     +-axes only: every dot product is exactly 1, 0 or -1, so pow(d, 128) is exact on both sides and the 0.98 threshold of the
              temporal pass is far away
  depths      one level per region, |1 - d / d'| >= 0.1 between any two levels (twice the temporal pass's 0.05), a ramp of at most
              2 % inside three of the regions, and one region of depth exactly 0 (pixel_distance_ratio = 0: the a-trous depth weight
              divides by its 1e-6 alone).  The HISTORY has no depth 0: 0 / 0 in the temporal pass would put a NaN weight into the
              moment plane, and non-finite propagation is not what these planes are for.
  colours     in [0, 2]: a step per region and per-pixel noise; contribs.w = 1.  Small on purpose: the variance is E[l^2] - E[l]^2
  motion      per region: zero, sub-pixel, whole-pixel and fractional vectors, two regions and two frame borders whose vectors leave
              the frame on the right, the bottom, the left and the top (clamp of prev_x / prev_y); |motion * size| stays below 2^20
  history     previous AOV planes of the same kind with the region cuts one pixel further, and moment planes whose frame counts
              1, 2, 3, 4, 7 change every 3 x 2 pixels: both branches of the variance pass (frame < 4 with radius 3 and 2, and
              the plain one) occur next to every frame edge
No NaN and no Inf anywhere.
"""
import numpy as np

SIZES = [(1, 1), (5, 3), (37, 21), (67, 33), (130, 1), (1, 70)]
FRAMES = (0, 1, 2, 3)

MESH_IDS = np.array([3, 0, 7, 1, 5, 2], np.float32)
NORMALS = np.array([(0, 0, 1), (1, 0, 0), (0, 1, 0), (-1, 0, 0), (0, -1, 0), (0, 0, -1)], np.float32)
DEPTH_LEVELS = np.array([1.0, 1.25, 2.0, 3.0, 0.0, 5.0], np.float32)        # region 4: depth exactly 0
HISTORY_DEPTH_LEVELS = np.array([1.0, 1.25, 2.0, 3.0, 0.5, 5.0], np.float32)
RAMPED = np.array([1, 0, 1, 0, 0, 1], np.float32)                          # regions whose depth carries the 2 % ramp
BASE_COLOUR = np.array([(0.3, 0.5, 0.9), (1.2, 0.8, 0.4), (0.6, 1.4, 0.7), (1.6, 1.1, 1.3), (0.9, 0.35, 1.0), (0.45, 1.7, 0.55)], np.float32)
ALBEDO = np.array([(0.8, 0.7, 0.6), (0.25, 0.9, 0.5), (1.0, 1.0, 1.0), (0.6, 0.3, 0.85), (0.5, 0.5, 0.5), (0.9, 0.2, 0.3)], np.float32)
BACKGROUND = np.array((0.7, 0.8, 1.0), np.float32)
NOISE = 0.25                # per-pixel colour noise, +-
FRAME_COUNTS = np.array([1, 2, 3, 4, 7], np.float32)
VARIANCE_FLOOR = 0.04       # least variance the history's moments encode


def _odd(v):
    return v | 1            # an odd cut is no multiple of 8, of 2 * 2^i or of 32


def _grid(w, h):
    return np.meshgrid(np.arange(w), np.arange(h))       # x[h, w], y[h, w]


def regions(w, h, shift=0):
    """Region index 0..5 per pixel: two stair-stepped column cuts and one row cut (`shift` moves the column cuts)."""
    x, y = _grid(w, h)
    c1, c2 = _odd((3 * w) // 7), _odd((5 * w) // 7)
    r1 = _odd((4 * h) // 9)
    xs = x + y // 3 + shift
    return ((xs >= c1).astype(np.int64) + (xs >= c2) + 3 * (y >= r1)).astype(np.int64)


def background(w, h, frame):
    """True where the pixel is background: singles, a run on the top row, a run on the right column, the bottom-left corner."""
    if w * h == 1:
        return np.full((1, 1), frame == 2)
    x, y = _grid(w, h)
    bg = (x * 7 + y * 13 + frame * 5) % 41 == 40
    bg |= (y == h - 1) & (x >= w // 3) & (x < w // 3 + max(2, w // 4))
    bg |= (x == w - 1) & (y >= h // 4) & (y < h // 4 + max(2, h // 3))
    bg |= (x == 0) & (y == 0)
    return bg


def _rng(w, h, frame, seed, stream):
    return np.random.default_rng([seed, w, h, frame, stream])


def _aovs(w, h, frame, reg, levels):
    x, y = _grid(w, h)
    bg = background(w, h, frame)
    nd = np.zeros((h, w, 4), np.float32)
    nd[..., :3] = NORMALS[(reg + (x + 2 * y) // 11) % 6]
    ramp = (np.float32(0.02) * (x + 2 * y).astype(np.float32) / np.float32(w + 2 * h)) * RAMPED[reg]
    nd[..., 3] = levels[reg] * (np.float32(1.0) + ramp)
    nd[bg] = (0.0, 0.0, 0.0, -1.0)
    am = np.zeros((h, w, 4), np.float32)
    am[..., :3] = ALBEDO[reg]
    am[..., 3] = MESH_IDS[reg]
    am[bg, :3] = BACKGROUND
    am[bg, 3] = -1.0
    return nd, am, bg


def _colours(w, h, reg, rng):
    c = BASE_COLOUR[reg] + rng.uniform(-NOISE, NOISE, (h, w, 3)).astype(np.float32)
    return np.clip(c, 0.0, 2.0).astype(np.float32)


def motion(w, h, frame, reg=None):
    """The external motion/depth plane (SetMotionDepthBuffer): motion.xy in screen fractions, depth, 1."""
    reg = regions(w, h) if reg is None else reg
    x, y = _grid(w, h)
    k = np.float32(1 + frame % 2)
    per_region = np.array([(0.0, 0.0), (0.4, -0.3), (2.0, 1.0), (-1.5, 2.5), (1.3 * w, 0.0), (0.0, -1.2 * h)], np.float32) * k
    px = per_region[reg]                                    # in pixels
    if w > 4:
        px[x < 2] = (-3.0, 0.5)                             # leaves the frame on the left ...
    if h > 4:
        px[y >= h - 2] = (0.25, 4.0)                        # ... and at the top
    md = np.zeros((h, w, 4), np.float32)
    md[..., 0] = px[..., 0] / np.float32(w)
    md[..., 1] = px[..., 1] / np.float32(h)
    md[..., 2] = DEPTH_LEVELS[reg]
    md[..., 3] = 1.0
    assert np.abs(md[..., 0] * w).max() < 2 ** 20 and np.abs(md[..., 1] * h).max() < 2 ** 20
    return md


def planes(w, h, frame, seed=0):
    """The four planes svgf_upload / Svgf.denoise take, and the motion plane, for one frame."""
    reg = regions(w, h)
    nd, am, bg = _aovs(w, h, frame, reg, DEPTH_LEVELS)
    x, y = _grid(w, h)
    contribs = np.ones((h, w, 4), np.float32)
    contribs[..., :3] = _colours(w, h, reg, _rng(w, h, frame, seed, 0))
    primary = np.zeros((h, w, 4), np.float32)
    primary[..., 0] = x; primary[..., 1] = y; primary[..., 2] = -nd[..., 3]; primary[..., 3] = 1.0
    primary[bg] = 0.0
    return dict(contribs=contribs, normal_depth=nd, albedo_meshid=am, primary_position=primary, motion_depth=motion(w, h, frame, reg))


def history(w, h, frame, seed=0):
    """The four previous AOV planes a frame > 0 starts from."""
    reg = regions(w, h, shift=1)
    nd, am, bg = _aovs(w, h, frame + 17, reg, HISTORY_DEPTH_LEVELS)
    x, y = _grid(w, h)
    rng = _rng(w, h, frame, seed, 1)
    cv = np.zeros((h, w, 4), np.float32)
    cv[..., :3] = _colours(w, h, reg, rng)
    cv[..., 3] = VARIANCE_FLOOR + 0.1 * rng.random((h, w), np.float32)
    n = FRAME_COUNTS[(x // 3 + 2 * (y // 2)) % 5]
    base = BASE_COLOUR[reg]
    mu = (0.2126 * base[..., 0] + 0.7152 * base[..., 1] + 0.0722 * base[..., 2]).astype(np.float32)
    s2 = (VARIANCE_FLOOR + 0.04 * rng.random((h, w), np.float32)).astype(np.float32)
    mt = np.zeros((h, w, 4), np.float32)
    mt[..., 0] = n * (mu * mu + s2)
    mt[..., 1] = n * mu
    mt[..., 2] = n
    mt[..., 3] = (1.0 + (x + y) % 9) / 9.0
    mt[bg] = (0.0, 0.0, 1.0, 1.0)           # what the variance pass leaves for a background pixel
    return dict(prev_normal_depth=nd, prev_albedo_meshid=am, prev_color_variance=cv, prev_moment_temporalweight=mt)


def perturbed(d, rng, names, rel=2.0 ** -18):
    """A copy of the plane dict `d` with every float of the planes in `names` moved by a random relative amount of up to `rel`.
    names: {plane: channels} -- ids and normals are never named."""
    out = {k: v.copy() for k, v in d.items()}
    for name, ch in names.items():
        p = out[name]
        f = (1.0 + rng.uniform(-rel, rel, p[..., ch].shape)).astype(np.float64)
        p[..., ch] = (p[..., ch].astype(np.float64) * f).astype(np.float32)
    return out


# what the conditioning test moves: colours, history colours and moments, depths
PERTURB_PLANES = {"contribs": slice(0, 3), "normal_depth": slice(3, 4), "motion_depth": slice(2, 3)}
PERTURB_HISTORY = {"prev_color_variance": slice(0, 4), "prev_moment_temporalweight": slice(0, 2), "prev_normal_depth": slice(3, 4)}


HISTORY_PLANES = ("prev_normal_depth", "prev_albedo_meshid", "prev_color_variance", "prev_moment_temporalweight")


def last_level_plane(iters):
    """The ping-pong plane the last of `iters` a-trous levels wrote: level i writes atrous[1 - (i & 1)]."""
    return "atrous%d" % (1 - ((iters - 1) & 1))


def oracle_frame(orc, cam, frame, pl, hist, iters=5, dilate=False):
    """One frame of the oracle's filter passes on the planes `pl` (planes()) from the history `hist` (history(); ignored at frame 0,
    which starts from freshly initialised buffers), on a renderer of its own so that frames do not depend on each other.
    Returns (before, after): `before` = every buffer the frame starts from that is not an input plane (what a GPU context has to be
    given to start from the same state; empty at frame 0), `after` = film, stages and the buffers the frame left."""
    sv = orc.Svgf()
    try:
        sv.set_atrous_iterations(iters)
        sv.set_dilate_temporal_weight(dilate)
        before = {}
        if frame > 0:
            for name in HISTORY_PLANES:
                sv.set_buffer(name, hist[name])
            before = {name: sv.buffer(name) for name in HISTORY_PLANES + ("color_variance", "moment_temporalweight")}
        sv.set_motion_depth(pl["motion_depth"])
        film, st = sv.denoise(cam, pl["contribs"], pl["normal_depth"], pl["albedo_meshid"], pl["primary_position"], frame=frame,
                              compute_motion=False, stages=True)
        after = {name: sv.buffer(name) for name in HISTORY_PLANES + ("temporary_color", "atrous0", "atrous1")}
        after["film"] = film
        after["stages"] = st
        return before, after
    finally:
        sv.close()
