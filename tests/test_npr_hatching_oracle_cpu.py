"""NPR hatching shadows on the CPU: the twin's filters (tests/cxx/npr_hatching_oracle.cpp) against closed forms worked out in float64,
and the library's new entry points.  docs/NPR_HATCHING.md has the decisions."""
import os
import subprocess

import numpy as np
import pytest

import npr_hatching_oracle as Hq
import npr_shadow_oracle as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("atn_npr_hatching_set", "atn_npr_hatching_get", "atn_npr_hatching_filter", "atn_npr_hatching_download")
INF = np.float32(np.inf)
DIRECTIONS = range(6)
STEP_TOL = 1e-6         # one step against float64: eleven float weights, two sums and a division on a value in [0, 1]


def test_library_exports_npr_hatching_entry_points():
    """The four atn_npr_hatching_* symbols: in the header, in the binding's list and in the built library's export table."""
    from aten_amd import _lib
    header = open(os.path.join(ROOT, "include", "aten_amd.h")).read()
    for s in SYMBOLS:
        assert "int %s(atn_ctx* ctx" % s in header, s
        assert s in _lib.SYMBOLS, s
    so = os.environ.get("ATEN_AMD_LIB") or os.path.join(ROOT, "aten_amd", "libaten_amd.so")
    out = subprocess.check_output(["nm", "-D", "--defined-only", so]).decode()
    names = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for s in SYMBOLS:
        assert s in names, s


def planes():
    """The test planes: 13x3, 7x2, 1x1 (every tap clamped), 37x4 with +inf depths -> (name, source, depth)."""
    rng = np.random.default_rng(23)
    out = []
    for w, h, misses in ((13, 3, 0.0), (7, 2, 0.0), (1, 1, 0.0), (37, 4, 0.25)):
        src = (rng.uniform(size=(h, w)) < 0.5).astype(np.float32)
        depth = rng.uniform(1.0, 1.6, (h, w)).astype(np.float32)
        miss = rng.uniform(size=(h, w)) < misses
        depth[miss] = INF
        src[miss] = 1.0
        out.append(("%dx%d" % (w, h), src, depth))
    return out


# ---- float64 closed forms: w = exp(-dist2 / 8 - (dc - d)^2 / dc); clamp(den > 0 ? num / den : 1, 0, 1)
def taps(line, x, y, w, h):
    """(dist2, tap x, tap y) of the 11 taps of a line: 1 row, 2 column, 3 diagonal, 6 anti-diagonal."""
    out = []
    for i in range(-5, 6):
        if line == 1:
            out.append((float(i * i), min(max(x + i, 0), w - 1), y))
        elif line == 2:
            out.append((float(i * i), x, min(max(y + i, 0), h - 1)))
        else:
            s = i if line == 3 else -i
            r = np.float64(np.float32(np.sqrt(np.float32(s * s + i * i))))     # the float square root, squared: not 2 i^2 exactly
            out.append((float(r * r), min(max(x + s, 0), w - 1), min(max(y + i, 0), h - 1)))
    return out


def step64(line, src, depth):
    h, w = src.shape
    out = np.ones((h, w), np.float64)
    for y in range(h):
        for x in range(w):
            c = np.float64(depth[y, x])
            if not np.isfinite(c):
                continue        # every weight NaN: 1
            num = den = 0.0
            for d2, tx, ty in taps(line, x, y, w, h):
                t = np.float64(depth[ty, tx])
                k = np.exp(-d2 / 8.0 - (c - t) ** 2 / c) if np.isfinite(t) else 0.0
                num += float(src[ty, tx]) * k
                den += k
            out[y, x] = min(max(num / den, 0.0), 1.0)
    return out


def want64(direction, src, depth):
    if direction == Hq.NONE:
        return src.astype(np.float64)
    if direction in (Hq.CROSS, Hq.ORTHOGONAL_CROSS):
        a = step64(1 if direction == Hq.CROSS else 3, src, depth)
        b = step64(2 if direction == Hq.CROSS else 6, src, depth)
        v = a * b
        return np.where(v < 1.0, 0.5 * v, v)
    return step64(direction, src, depth)


@pytest.mark.parametrize("name,src,depth", planes(), ids=[p[0] for p in planes()])
def test_every_direction_against_float64(name, src, depth):
    """All six directions (and the anti-diagonal alone) on the small planes, every pixel: clamped taps, +inf depths (a miss-centred
    pixel is exactly 1, a miss tap under a hit centre weighs 0)."""
    miss = np.isinf(depth)
    for direction in list(DIRECTIONS) + [Hq.ANTI_DIAGONAL]:
        got = Hq.filter(src, depth, direction)
        if direction == Hq.NONE:
            assert np.array_equal(got, src)
            continue
        want = want64(direction, src, depth) if direction != Hq.ANTI_DIAGONAL else step64(6, src, depth)
        two_step = direction in (Hq.CROSS, Hq.ORTHOGONAL_CROSS)
        assert np.all(got[miss] == 1.0), (name, direction)
        # (a product that float64 puts on the other side of 1 than the twin would be halved on one side only: none here -- checked)
        assert np.abs(got - want).max() <= (2.5 if two_step else 1.0) * STEP_TOL, (name, direction, np.abs(got - want).max())
    if src.shape == (1, 1):
        for direction in (1, 2, 3):
            assert np.array_equal(Hq.filter(src, depth, direction), src)       # eleven taps of the one pixel


def test_all_lit_is_exactly_one_and_is_not_halved():
    rng = np.random.default_rng(5)
    depth = rng.uniform(0.5, 9.0, (4, 37)).astype(np.float32)
    depth[1, 7] = depth[3, 30] = INF
    one = np.ones_like(depth)
    for direction in DIRECTIONS:
        out, first = Hq.filter(one, depth, direction, first=True)
        assert np.array_equal(out, one), direction         # numerator and denominator are the same sum; 1 * 1 is not < 1
        assert np.array_equal(first, one), direction


def test_horizontal_is_the_shadow_twins_row_filter():
    for _, src, depth in planes():
        assert np.array_equal(Hq.filter(src, depth, Hq.HORIZONTAL), S.row_filter(src, depth))


def test_vertical_is_horizontal_transposed():
    """A vertical lit step at uniform depth."""
    n = 40
    lit = (np.arange(n) >= 20).astype(np.float32)
    rows = np.repeat(lit[None, :], 3, 0)            # [3, 40]: the step along x
    cols = np.ascontiguousarray(rows.T)             # [40, 3]: the step along y
    h = Hq.filter(rows, np.full_like(rows, 3.25), Hq.HORIZONTAL)
    v = Hq.filter(cols, np.full_like(cols, 3.25), Hq.VERTICAL)
    assert np.array_equal(v, h.T)
    assert v[14, 1] == 0.0 and v[25, 1] == 1.0 and 0.0 < v[19, 1] < 0.5 < v[20, 1] < 1.0
    # and on random planes with misses, tap for tap
    for _, src, depth in planes():
        assert np.array_equal(Hq.filter(np.ascontiguousarray(src.T), np.ascontiguousarray(depth.T), Hq.VERTICAL),
                              Hq.filter(src, depth, Hq.HORIZONTAL).T)


def test_orthogonal_diagonal_step():
    """lit = (x + y >= 40) at one depth: along the diagonal (x + h, y + h) the sum rises by 2 per tap; the weights are
    exp(-(sqrt(2 h^2))^2 / 8) with the square root rounded to float."""
    n = 40
    yy, xx = np.mgrid[0:n, 0:n]
    lit = (xx + yy >= 40).astype(np.float32)
    out = Hq.filter(lit, np.full_like(lit, 2.0), Hq.ORTHOGONAL)

    def g(h):
        r = np.float64(np.float32(np.sqrt(np.float32(2 * h * h))))
        return np.exp(-(r * r) / 8.0)
    g_all = sum(g(h) for h in range(-5, 6))
    for y in range(5, n - 5):
        for x in range(5, n - 5):
            want = sum(g(h) for h in range(-5, 6) if x + y + 2 * h >= 40) / g_all
            assert abs(float(out[y, x]) - want) <= STEP_TOL, (x, y)
    assert float(np.float32(np.sqrt(np.float32(2 * 3 * 3)))) ** 2 != 18.0      # the float square is not 2 h^2


def test_cross_at_uniform_depth_is_half_the_product():
    rng = np.random.default_rng(9)
    src = (rng.uniform(size=(12, 31)) < 0.6).astype(np.float32)
    src[3:9, 10:28] = 1.0       # a region whose windows are all lit: the product is exactly 1 and is not halved
    depth = np.full_like(src, 2.5)
    cross, first = Hq.filter(src, depth, Hq.CROSS, first=True)
    hz, vt = Hq.filter(src, depth, Hq.HORIZONTAL), Hq.filter(src, depth, Hq.VERTICAL)
    assert np.array_equal(first, hz)
    prod = vt * hz      # float32, the twin's order: the second step's value times the first's
    below = prod < 1.0
    assert below.sum() > 100 and (~below).sum() >= 1
    assert np.array_equal(cross[below], (prod * np.float32(0.5))[below])
    assert np.all(cross[~below] == 1.0)
    assert np.abs(cross[below] - 0.5 * hz.astype(np.float64)[below] * vt[below]).max() <= 1e-7


def test_anti_diagonal_is_the_diagonal_mirrored_in_x():
    for _, src, depth in planes():
        mirrored = Hq.filter(np.ascontiguousarray(src[:, ::-1]), np.ascontiguousarray(depth[:, ::-1]), Hq.ORTHOGONAL)
        assert np.array_equal(Hq.filter(src, depth, Hq.ANTI_DIAGONAL), mirrored[:, ::-1])
    # and through the product: OrthogonalCross of a plane is OrthogonalCross of its mirror image, mirrored, up to the order of the
    # two factors -- which a float product does not see
    _, src, depth = planes()[3]
    a = Hq.filter(src, depth, Hq.ORTHOGONAL_CROSS)
    b = Hq.filter(np.ascontiguousarray(src[:, ::-1]), np.ascontiguousarray(depth[:, ::-1]), Hq.ORTHOGONAL_CROSS)[:, ::-1]
    assert np.array_equal(a, b)


def test_none_returns_the_source_bit_for_bit():
    src = np.float32([[0.0, 1.7, 0.25, -0.5], [1.0, 3.0e-41, 0.999, 1.7]])       # above 1, below 0, a denormal: kept as written
    depth = np.float32([[1.0, INF, 2.0, 1.0], [INF, 1.0, 1.0, 1.0]])
    out, first = Hq.filter(src, depth, Hq.NONE, first=True)
    assert np.array_equal(out.view(np.uint32), src.view(np.uint32))
    assert np.array_equal(first.view(np.uint32), src.view(np.uint32))
