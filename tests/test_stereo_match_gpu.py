"""The stereo kernel (stereo_lk_sized_kernel, gf_stereo_kernels.hpp) through its building block gf_stereo_match_batch against oracle_py.lk, bit for bit: right
points, status and forward status of every point -- on the scenes of tests/stereo_ref.py at both sizes and on the pairs of tests/lk_hard_cases.py taken as (left,
right), so that every exit of an LK level pass is taken in both directions; as one batch, one pair at a time, and twice.  Run with -m gpu."""
import numpy as np
import pytest

import lk_hard_cases as L
import roi_ref as RR
import stereo_ref as SR

pytestmark = pytest.mark.gpu

_REF = {}


def _scene_batch(oracle, case):
    """the six (left, right) pairs of a size with the points the tracker would hand the stage: cur_pts of every frame, survivors first, then the new corners"""
    if case not in _REF:
        w, h, max_cnt, min_dist = case
        left, right = SR.scene(w, h)
        o = oracle.Tracker(oracle.default_cfg(max_cnt=max_cnt, min_dist=min_dist, flow_back=1, depth_cam=0))
        pts = []
        for k in range(SR.K):
            o.track(0.0666 * k, left[k], None)
            pts.append(o.state()[2].copy())
        flow_back = [1, 0, 1, 1, 0, 1]
        ref = [SR.match(oracle, left[k], right[k], pts[k], flow_back[k])[:3] for k in range(SR.K)]
        for r in ref:
            for a in r:
                a.setflags(write=False)
        _REF[case] = (left, right, pts, flow_back, ref)
    return _REF[case]


HARD = ["block2_shift", "block2_inverse", "cells_small_shift", "cells_large_shift", "pixel_noise_shift", "pixel_noise_fresh", "mixed_checker_cells", "quilt"]   # 176 x 192


def _hard_batch(oracle, names):
    key = tuple(names)
    if key not in _REF:
        cs = [next(c for c in L.cases() if c["name"] == n) for n in names]
        ref = [SR.match(oracle, c["prev"], c["next"], c["pts"], 1)[:3] for c in cs]
        _REF[key] = (cs, ref)
    return _REF[key]


def _same(ref, got, what):
    for k, ((r_pts, r_st, r_fwd), (g_pts, g_st, g_fwd)) in enumerate(zip(ref, got)):
        assert np.array_equal(r_fwd, g_fwd), "%s, pair %d: forward status differs at points %s" % (what, k, np.nonzero(r_fwd != g_fwd)[0][:12])
        assert np.array_equal(r_st, g_st), "%s, pair %d: status differs at points %s" % (what, k, np.nonzero(r_st != g_st)[0][:12])
        bad = np.nonzero((r_pts.view(np.uint32) != g_pts.view(np.uint32)).any(axis=1))[0]
        assert len(bad) == 0, "%s, pair %d: right points differ at points %s (forward status %s)" % (what, k, bad[:12], r_fwd[bad[:12]])
    assert len(ref) == len(got)


@pytest.mark.parametrize("case", SR.CASES, ids=RR.size_id)
def test_scenes_as_one_batch_one_at_a_time_and_twice(gf, oracle, case):
    left, right, pts, flow_back, ref = _scene_batch(oracle, case)
    kept = sum(int(r[1].sum()) for r in ref)
    assert 4 * kept >= sum(len(p) for p in pts) and any((r[1] != r[2]).any() for r in ref)   # not vacuous: points are kept, and the reverse check drops some
    batch = gf.stereo_match(left, right, pts, flow_back)
    _same(ref, batch, "one batch")
    _same(ref, gf.stereo_match(left, right, pts, flow_back), "the batch again")
    for k in range(SR.K):
        _same(ref[k:k + 1], gf.stereo_match(left[k:k + 1], right[k:k + 1], pts[k:k + 1], flow_back[k]), "pair %d alone" % k)


def test_hard_cases_both_directions(gf, oracle):
    cs, ref = _hard_batch(oracle, HARD)
    census = [oracle.lk_census(c["prev"], c["next"], c["pts"], None, max_level=3)[3] for c in cs]
    back = [oracle.lk_census(c["next"], c["prev"], r[0][r[2] > 0], None, max_level=3)[3] for c, r in zip(cs, ref)]   # the kernel runs the reverse pass where the forward one held
    # template_out cannot occur in a reverse pass: its template window sits on the right point, which a forward pass that held left inside the search range
    for name, ex, never in (("forward", census, set()), ("reverse", back, {oracle.LK_EXITS.index("template_out")})):
        seen = set(np.concatenate([e.reshape(-1) for e in ex]).tolist()) - {0}
        assert seen == set(range(1, len(oracle.LK_EXITS))) - never, "%s passes take exits %s only" % (name, sorted(seen))
    assert sum(int(r[1].sum()) for r in ref) > 200
    got = gf.stereo_match([c["prev"] for c in cs], [c["next"] for c in cs], [c["pts"] for c in cs], 1)
    _same(ref, got, "hard cases")
    _same(ref[2:3], gf.stereo_match([cs[2]["prev"]], [cs[2]["next"]], [cs[2]["pts"]], 1), "cells_small_shift alone")


def test_three_level_pyramid_and_odd_lists(gf, oracle):
    """160 x 120 has three levels (maxLevel 3 is cut to 2); lists of 1 mod 4 points, of one point and of none beside a full one"""
    cs, ref = _hard_batch(oracle, ["quilt_three_levels"])
    c = cs[0]
    n = len(c["pts"]) - 3
    assert n % 4 == 1
    lists = [c["pts"][:n], c["pts"][5:6], c["pts"][:0], c["pts"]]
    want = [SR.match(oracle, c["prev"], c["next"], p, fb)[:3] for p, fb in zip(lists, (1, 1, 1, 0))]
    got = gf.stereo_match([c["prev"]] * 4, [c["next"]] * 4, lists, [1, 1, 1, 0])
    _same(want, got, "three levels")
    assert len(got[2][0]) == 0


def test_device_form_and_refusals(gf, oracle):
    import torch
    case = SR.CASES[1]
    left, right, pts, flow_back, ref = _scene_batch(oracle, case)
    dl, dr = torch.from_numpy(np.stack(left)).cuda(), torch.from_numpy(np.stack(right)).cuda()
    got = gf.stereo_match_device(dl.data_ptr(), dr.data_ptr(), SR.K, case[0], case[1], pts, flow_back)
    _same(ref, got, "device frames")
    with pytest.raises(gf.GfError, match="4-byte"):
        gf.stereo_match_device(dl.data_ptr() + 1, dr.data_ptr(), SR.K, case[0], case[1], pts, flow_back)
    with pytest.raises(gf.GfError):
        gf.stereo_match([left[0][:, :62]], [right[0][:, :62]], pts[:1], 1)      # a width that is no multiple of 4
