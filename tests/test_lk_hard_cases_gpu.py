"""The LK kernels, the detector and the whole tracker against the CPU oracle on the hard-case inputs of tests/lk_hard_cases.py: binary frames that take every exit of
lk_level at every level, drive the exact sums past 2^32 and put points with different exits next to each other in a wavefront (what the inputs reach is held by
tests/test_lk_hard_cases_host.py on the CPU).  Bit-exact, in all three kernel forms.  Run with -m gpu."""
import numpy as np
import pytest
import lk_hard_cases as L

pytestmark = pytest.mark.gpu

CASE_NAMES = list(L.CASE_NAMES)
KERNELS = [None, "2", "4"]   # GF_LK_POINTS: unset (lk_track_kernel), lk_track_mp_kernel<2>, lk_track_mp_kernel<4>
_REF = {}


def _case(name):
    return next(c for c in L.cases() if c["name"] == name)


def _reference(oracle, name):
    """the oracle's result of a case, computed once and shared (never written to)"""
    if name not in _REF:
        c = _case(name)
        pts, st, it = oracle.lk(c["prev"], c["next"], c["pts"], c["init"], max_level=c["max_level"])
        pts.setflags(write=False); st.setflags(write=False)
        _REF[name] = (pts, st, it)
    return _REF[name]


def _kernel(monkeypatch, points):
    if points is None:
        monkeypatch.delenv("GF_LK_POINTS", raising=False)
    else:
        monkeypatch.setenv("GF_LK_POINTS", points)


def _contract(ref, got, what):
    """status of every point, the total iteration count, and the coordinates of every status-1 point as uint32"""
    (r_pts, r_st, r_it), (g_pts, g_st, g_it) = ref, got
    assert np.array_equal(r_st, g_st), "%s: status differs at points %s" % (what, np.nonzero(r_st != g_st)[0][:12])
    assert r_it == g_it, "%s: %d iterations, the oracle ran %d" % (what, g_it, r_it)
    ok = r_st > 0
    bad = np.nonzero((r_pts.view(np.uint32) != g_pts.view(np.uint32)).any(axis=1) & ok)[0]
    assert len(bad) == 0, "%s: coordinates differ at points %s" % (what, bad[:12])


@pytest.mark.parametrize("points", KERNELS)
@pytest.mark.parametrize("name", CASE_NAMES)
def test_lk_hard_case_bit_exact(gf, oracle, monkeypatch, name, points):
    _kernel(monkeypatch, points)
    c = _case(name)
    ref = _reference(oracle, name)
    assert 3 * int(ref[1].sum()) >= len(ref[1])     # the coordinate comparison is not vacuous
    _contract(ref, gf.lk_track(c["prev"], c["next"], c["pts"], c["init"], max_level=c["max_level"]), name)


@pytest.mark.parametrize("points", KERNELS)
@pytest.mark.parametrize("name", ["block2_shift", "cells_large_shift", "quilt", "quilt_predicted", "quilt_edge_start"])
def test_lk_results_do_not_depend_on_the_neighbours_in_a_wavefront(gf, oracle, monkeypatch, name, points):
    """the same points in a seeded shuffled order give the same results, permuted; so does a list cut to a length of 1 mod 4 (the last wavefront of the multi-point
    kernels holds one point).  Points are independent in the reference; in the kernels P of them share a wavefront and a level pass runs as long as the slowest."""
    _kernel(monkeypatch, points)
    c = _case(name)
    r_pts, r_st, _ = _reference(oracle, name)
    n = len(c["pts"])
    _, _, _, exits, _, _, _ = oracle.lk_census(c["prev"], c["next"], c["pts"], c["init"], max_level=c["max_level"])
    iters_of = lambda sel: oracle.lk(c["prev"], c["next"], c["pts"][sel], None if c["init"] is None else c["init"][sel], max_level=c["max_level"])[2]
    perm = np.random.default_rng(11).permutation(n)
    cut = np.arange(n - 3)
    assert len(cut) % 4 == 1
    for what, sel in (("shuffled", perm), ("1 mod 4", cut)):
        got = gf.lk_track(c["prev"], c["next"], c["pts"][sel], None if c["init"] is None else c["init"][sel], max_level=c["max_level"])
        _contract((r_pts[sel], r_st[sel], iters_of(sel)), got, "%s, %s" % (name, what))
    assert len(set(exits[:, 0].tolist())) >= 4      # the list mixes at least four level-0 exits


@pytest.mark.parametrize("frame", ["block2", "cells", "mixed"])
def test_detector_on_periodic_binary_frames(gf, oracle, frame):
    """min_eigen_val and good_features on frames with thousands of exactly equal eigenvalues, across the strip boundaries of the Shi-Tomasi pass: the tie rule
    (the larger offset first) decides the order of almost every candidate"""
    img = dict(L.detector_frames())[frame]
    a, b = oracle.min_eigen_val(img), gf.min_eigen_val(img)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    counts = np.unique(a[a > 0], return_counts=True)[1]
    assert counts.max() >= 100, "the frame has no large set of equal eigenvalues"
    for min_dist in (3, 12):
        ca = oracle.good_features(img, 400, min_dist=float(min_dist))
        cb = gf.good_features(img, 400, min_dist=min_dist)
        assert len(ca) > 40
        assert len(ca) == len(cb) and np.array_equal(ca, cb), (frame, min_dist)


@pytest.mark.parametrize("points", [None, "4"])
def test_tracker_on_cell_noise_sequences(gf, oracle, monkeypatch, points):
    """six frames of trackImage on 320 x 240 cell noise (grey levels 0 / 250, one frame pair at 255 where the brightness test drops every track on a bright pixel),
    max_cnt 150, min_dist 12, flow_back 1: ids and observations bit for bit against the oracle's tracker -- alone, and as sequence 0 of a batch of two whose
    sequence 1 sees the checkerboard | cell-noise frames"""
    _kernel(monkeypatch, points)
    seq0, seq1 = L.tracker_sequences()
    kw = dict(max_cnt=150, min_dist=12, flow_back=1, depth_cam=0)
    ref = []
    for seq in (seq0, seq1):
        otr = oracle.Tracker(oracle.default_cfg(**kw))
        ref.append([otr.track(0.0666 * k, f, None) for k, f in enumerate(seq)])
        assert otr.lk_iters() > 10000
    assert all(len(ids) == 150 for ids, _ in ref[0])
    kept = [len(set(ref[0][k][0].tolist()) & set(ref[0][k + 1][0].tolist())) for k in range(5)]
    assert min(kept) >= 60 and max(kept) >= 140 and min(kept) <= 100, kept     # tracks survive; the frames at 255 drop a good third of them
    gtr = gf.FeatureTracker(gf.default_cfg(width=L.TW, height=L.TH, **kw))
    for k, f in enumerate(seq0):
        gi, go = gtr.trackImage(0.0666 * k, f, None)
        assert np.array_equal(ref[0][k][0], gi), "frame %d: feature id lists differ" % k
        assert np.array_equal(ref[0][k][1].view(np.uint64), go.view(np.uint64)), "frame %d: observations differ" % k
    gtr.close()
    gtr = gf.FeatureTracker(gf.default_cfg(width=L.TW, height=L.TH, batch=2, **kw))
    for k in range(len(seq0)):
        res = gtr.trackImageBatch([0.0666 * k] * 2, [seq0[k], seq1[k]], None)
        for b in range(2):
            assert np.array_equal(ref[b][k][0], res[b][0]), "frame %d, sequence %d: feature id lists differ" % (k, b)
            assert np.array_equal(ref[b][k][1].view(np.uint64), res[b][1].view(np.uint64)), "frame %d, sequence %d: observations differ" % (k, b)
    gtr.close()
