"""The sets behind tests/test_gpu_volume_nested.py, pinned on the CPU twin (tests/cxx/volume_oracle.cpp) so that the GPU tests cannot
pass by being empty: the first-decision masks of the nested scenes hold events at every stack depth, the first-medium scene holds
almost none, the overflow scenes overflow, no compared pixel sits on a near tie, and the twin's stack equals a hand-worked one.
Scenes, masks and the cases: tests/volume_scenes.py."""
import numpy as np
import pytest

import volume_oracle as V
import volume_scenes as VS


@pytest.fixture(scope="module")
def orc():
    from oracle import orc as o
    o.lib()
    V.lib()
    return o


W0, H0 = VS.SIZES[0]
STAGE_CASES = [(name, n) for name, n in (("thin", 8), ("thin", 12), ("outer_dense", 8), ("outer_thin", 8))]


@pytest.mark.parametrize("frame", VS.FRAMES)
def test_outer_dense_decides_at_every_stack_depth(orc, frame):
    c = VS.case(orc, V, "outer_dense", 8, W0, H0, frame)
    for k in range(1, VS.ITERATIONS):
        m = c["masks"][k]
        ev = int((VS.events(c["stages"][k]) & m).sum())
        print("outer_dense frame %d iteration %d: %d first-decision pixels, %d events" % (frame, k, m.sum(), ev))
        assert ev >= 20
        assert m.sum() >= 100
        # a first decision at k is taken with up to k media on the stack, and the deepest stack is reached
        assert c["stages"][k - 1]["state"]["stack_size"][m].max() == k
    # the connections of iteration 0 start at exact floor hits and cross the shells on their way to the light
    st0 = c["stages"][0]
    deep = st0["state"]["connection"] & (st0["conn"]["segments"] >= 3)
    assert deep.sum() >= 1000
    assert max(int(st["conn"]["segments"].max()) for st in c["stages"]) == 9
    assert c["counters"]["stack_overflow"] == 0 and c["counters"]["walk_overflow"] == 0


@pytest.mark.parametrize("frame", VS.FRAMES)
def test_the_ragged_size_decides_at_every_stack_depth_too(orc, frame):
    """37 x 21 has a quarter of the pixels: the floors are its own (the counts of 64 x 48 scaled down and rounded down)."""
    w, h = VS.SIZES[1]
    c = VS.case(orc, V, "outer_dense", 8, w, h, frame)
    for k in range(1, VS.ITERATIONS):
        m = c["masks"][k]
        assert m.sum() >= 10
        assert (VS.events(c["stages"][k]) & m).sum() >= 3


def test_outer_thin_pins_the_first_medium_rule(orc):
    """The current medium is the first entered (sigma_t 1e-3), not the newest (sigma_t 5.5): events on at most 1 % of the
    first-decision pixels, where a renderer that sampled the newest medium would scatter most of them."""
    for w, h in VS.SIZES:
        for frame in VS.FRAMES:
            c = VS.case(orc, V, "outer_thin", 8, w, h, frame)
            px = sum(int(m.sum()) for m in c["masks"][1:])
            ev = sum(int((VS.events(st) & m).sum()) for st, m in zip(c["stages"][1:], c["masks"][1:]))
            deep = sum(int((st["state"]["stack_size"][m] >= 2).sum()) for st, m in zip(c["stages"][:-1], c["masks"][1:]))
            print("outer_thin %d x %d frame %d: %d events on %d first-decision pixels, %d of them under two media or more" % (w, h, frame, ev, px, deep))
            assert ev <= px / 100
            assert deep >= px / 2


def test_thin_twelve_fills_and_overflows_the_stack(orc):
    for w, h in VS.SIZES:
        for frame in VS.FRAMES:
            c = VS.case(orc, V, "thin", 12, w, h, frame, max_depth=VS.COUNTER_MAX_DEPTH)
            full = c["masks"][7] & (c["stages"][7]["state"]["stack_size"] == 8)
            assert full.sum() >= 20
            assert c["counters"]["stack_overflow"] > 0 and c["counters"]["walk_overflow"] == 0
            assert not any(VS.events(st).any() for st in c["stages"])


@pytest.mark.parametrize("m,over", [(33, True), (32, False)])
def test_slab_row_reaches_the_walk_bound(orc, m, over):
    """2 m boundaries per connection: 64 are walked (65 segments), the 65th boundary ends the walk as blocked and is counted."""
    for w, h in VS.SIZES:
        for frame in VS.FRAMES:
            c = VS.case(orc, V, "slab_row", m, w, h, frame, max_depth=VS.COUNTER_MAX_DEPTH)
            st0 = c["stages"][0]
            assert st0["state"]["connection"].all()
            assert np.all(st0["conn"]["segments"] == 65)
            assert np.all(st0["conn"]["visible"] == (not over))
            assert (c["counters"]["walk_overflow"] >= w * h) if over else (c["counters"]["walk_overflow"] == 0)
            assert c["counters"]["stack_overflow"] == 0
            assert max(int(st["state"]["stack_size"].max()) for st in c["stages"]) == 1


def test_the_dense_slab_row_attenuates(orc):
    """Beer-Lambert along the connection, by hand: 32 slabs of sigma_t 0.5, 0.05 thick, crossed at the connection's slant."""
    w, h = VS.SIZES[0]
    c = VS.case(orc, V, "slab_row_dense", 32, w, h, 0)
    st0 = c["stages"][0]
    assert st0["state"]["connection"].all() and st0["conn"]["visible"].all()
    d = st0["conn"]["dir"].astype(np.float64)
    want = np.exp(-0.5 * 32 * 0.05 / np.abs(d[..., 2]))
    # (ray_offset moves every boundary crossing by ~1e-3 relative of a slab's thickness)
    np.testing.assert_allclose(st0["conn"]["transmittance"], want, rtol=2e-3)


def counter_cases():
    return [("thin", 12)] + [("slab_row", 33), ("slab_row", 32)]


@pytest.mark.parametrize("name,n", counter_cases())
def test_under_the_counter_setting_every_connection_starts_behind_passes_only(orc, name, n):
    """max_depth = 1 and media without events: every connection of the frame is made at the first surface a path meets, on a
    first-decision pixel, so its record is bit-equal on the device and the frame's connection counters are exact there."""
    for w, h in VS.SIZES:
        for frame in VS.FRAMES:
            c = VS.case(orc, V, name, n, w, h, frame, max_depth=VS.COUNTER_MAX_DEPTH)
            total = seg = 0
            for st, m in zip(c["stages"], c["masks"]):
                conn = st["state"]["connection"]
                assert not (conn & ~m).any()
                total += int(conn.sum())
                seg += int(st["conn"]["segments"][conn].sum())
            assert total == c["counters"]["connections"] and total > 0
            assert seg == c["counters"]["segments"]


@pytest.mark.parametrize("name,n", STAGE_CASES + [("slab_row_dense", 33), ("slab_row_dense", 32)])
def test_no_compared_pixel_sits_on_a_near_tie(orc, name, n):
    """Every scene, size, frame and iteration the GPU tests use: no first-decision pixel whose sampled distance lies within 4 ulp of
    the hit distance.  So the GPU tests leave no pixel out."""
    for w, h in VS.SIZES:
        for frame in VS.FRAMES:
            for kw in ((dict(), dict(max_depth=VS.COUNTER_MAX_DEPTH)) if (name, n) == ("thin", 12) else (dict(),)):
                c = VS.case(orc, V, name, n, w, h, frame, **kw)
                for k, (st, m) in enumerate(zip(c["stages"], c["masks"])):
                    assert VS.near_ties(st, m).sum() == 0, (name, n, w, h, frame, k)


@pytest.mark.parametrize("n", (8, 12))
def test_thin_stack_by_hand(orc, n):
    """The twin's stack on pass-only pixels against shells_by_hand (ray / box arithmetic in float64, a Python list as the stack):
    the shell ids 0 .. k-1 in entry order going in, shortened from the newest end going out, never more than eight."""
    for w, h in VS.SIZES:
        for frame in VS.FRAMES:
            c = VS.case(orc, V, "thin", n, w, h, frame)
            assert c["ids"] == sorted(c["ids"]) and len(set(c["ids"])) == n
            rays = orc.generate_paths(c["cam"], c["seeds"], w, h, 0, frame)
            passes, stacks, sizes, clear = VS.shells_by_hand(rays["org"], rays["dir"], c["ids"], n)
            passes, stacks, sizes, clear = passes.reshape(h, w), stacks.reshape(h, w, 8, 8), sizes.reshape(h, w, 8), clear.reshape(h, w)
            assert (~clear).sum() <= w * h / 100
            deepest = 0
            for k, st in enumerate(c["stages"]):
                po = c["masks"][k] & VS.pass_only(st) & clear
                assert np.array_equal(po, (passes > k) & clear), k
                assert np.array_equal(st["state"]["stack_size"][po], sizes[..., k][po]), k
                assert np.array_equal(st["stack"][po], stacks[..., k, :][po]), k
                assert np.all(st["state"]["depth_count"][po] == 0)
                if po.any():
                    deepest = max(deepest, int(sizes[..., k][po].max()))
            assert deepest == 8
            # both ways are seen: stacks that grow and stacks that shrink again
            last = c["masks"][7] & VS.pass_only(c["stages"][7])
            assert (sizes[..., 7][last] < sizes[..., 6][last]).any() and (sizes[..., 7][last] > sizes[..., 6][last]).any()


def test_first_decision_masks_by_hand():
    def st(processed, passed, scattered=0, absorbed=0):
        b = lambda v: np.array([[(v >> i) & 1 for i in range(4)]], bool)
        return dict(state=dict(processed=b(processed), passed=b(passed), scattered=b(scattered), absorbed=b(absorbed)))
    # pixel 0 passes twice; pixel 1 scatters at 0; pixel 2 passes then is absorbed; pixel 3 is never processed
    masks = VS.first_decision_masks([st(0b0111, 0b0101, scattered=0b0010), st(0b0111, 0b0001, absorbed=0b0100), st(0b0111, 0b0000)])
    assert [m[0].tolist() for m in masks] == [[True, True, True, False], [True, False, True, False], [True, False, False, False]]
