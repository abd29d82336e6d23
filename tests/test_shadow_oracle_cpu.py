"""The oracle's shadow-ray entry (orc.shadow_visible: HitTestToTargetLight per query) and the ray sets of the per-ray visibility gate
(tests/shadow_rays.py), without a GPU:

  * in scenes where no surface can be ignored the verdict equals scene::hitLight restated in NumPy over orc.trace_closest;
  * in the pane stack it follows from counting panes against the lookup budget (1, or 10 with alpha blending or the stencil flag);
  * in every case both verdicts occur in at least 5 % of each category's rays -- a condition on the inputs, asserted here and again
    where the GPU runs them (tests/test_gpu_shadow_rays.py).  The stacks of 10 and 11 panes towards the point light can only be
    blocked where a ray crosses all panes: their rays that pass beside the stack keep the share up, so they are held to the floor too."""
import numpy as np
import pytest

import shadow_rays as S

OPAQUE = [k for k, v in S.CASES.items() if v[2]]
OTHER = [k for k, v in S.CASES.items() if not v[2]]


@pytest.mark.parametrize("name", OPAQUE)
def test_opaque_scene_verdict_is_hit_light_over_the_closest_hit(orc, cornell, name):
    fs, _, rs, vis = S.case(orc, name, cornell)
    assert not np.any(fs.arrays["materials"]["stencil_type"]) and fs.desc.config.enable_alpha_blending == 0
    want, _ = S.restate_opaque(orc, fs, rs)
    assert np.array_equal(vis, want), S.mismatch_report(rs, vis, want)
    S.check_floor(rs, vis, name)
    assert set(c[0] for c in rs.cat) == set(S.CASES[name][1])


@pytest.mark.parametrize("name,k,blending,lamp", S.STACKS)
def test_pane_stack_verdict_follows_from_counting_panes(orc, name, k, blending, lamp):
    fs, _, rs, vis = S.case(orc, name)
    assert S.pane_count(fs) == k
    want, decided = S.pane_stack_verdict(orc, fs, rs, blending)
    assert decided.mean() > 0.2
    assert np.array_equal(vis[decided], want[decided]), S.mismatch_report(rs.take(decided), vis[decided], want[decided])
    S.check_floor(rs, vis, name)
    vis2, lookups, last = orc.shadow_visible(fs, rs.queries(orc), details=True)
    assert np.array_equal(vis2, vis)
    budget = np.where(rs.stencil | bool(blending), 10, 1)
    assert np.all(lookups >= 1) and np.all(lookups <= budget)
    crossing = lookups > 1
    if blending or k < 10:
        # some rays end in a miss after ignored hits ...
        assert np.any(crossing & (last["objid"] < 0)) == (k + (2 if lamp else 1) <= 10 or lamp)
    # ... and some on an opaque blocker after them (the strip, or an opaque texel of a later pane)
    assert np.any(crossing & (last["objid"] >= 0) & (vis == 0))
    if k >= 10:
        assert lookups.max() == 10      # the budget is reached


@pytest.mark.parametrize("name", [k for k in OTHER if k.startswith("room")])
def test_stencil_room_has_both_verdicts_with_and_without_the_flag(orc, name):
    fs, _, rs, vis = S.case(orc, name)
    S.check_floor(rs, vis, name)
    _, lookups, last = orc.shadow_visible(fs, rs.queries(orc), details=True)
    assert lookups.max() >= 3                               # restarts behind ignored surfaces do happen
    assert np.any((lookups > 1) & (last["objid"] < 0)) and np.any((lookups > 1) & (last["objid"] >= 0))
    on, off = rs.cat == "D room flag on", rs.cat == "D room flag off"
    assert on.sum() == off.sum() and np.array_equal(rs.org[on], rs.org[off])
    if name.endswith("noblend"):
        assert np.any(vis[on] != vis[off])                  # the flag alone raises the budget from 1 to 10: it decides some rays


def test_entry_rejects_a_light_index_outside_the_scene(orc, cornell):
    fs, _ = cornell
    q = orc.shadow_queries([[0, 1, 0]], [[0, 1, 0]], 1.0, 1)
    with pytest.raises(ValueError):
        orc.shadow_visible(fs, q)
    assert len(orc.shadow_visible(fs, q[:0])) == 0


def test_builders_are_deterministic(orc, cornell):
    fs, cam = cornell
    a = S.category_c(orc, fs, 0, S.surface_points(orc, fs, cam))
    b = S.category_c(orc, fs, 0, S.surface_points(orc, fs, cam))
    assert a.org.tobytes() == b.org.tobytes() and a.dir.tobytes() == b.dir.tobytes() and a.dist.tobytes() == b.dist.tobytes()
