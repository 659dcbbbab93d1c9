"""Stereo depth in the tracker (gf_tracker_set_seq_stereo_depth): the observations of tests/stereo_ref.py's Tracker with the eighth field of the LEFT ones replaced
by the restatement of tests/stereo_depth_ref.py applied to that frame's cur_pts / right points / status, bit for bit; right_obs 0 drops the camera-1 entries; every
other field, ids, n_out, state and the stereo stage's counters stay what test_stereo_tracker_gpu.py pins.  One handle carries a stereo sequence with depth and
right_obs 1, one with depth and right_obs 0, a stereo sequence without depth and (in one variant) a mono sequence.  Run with -m gpu."""
import numpy as np
import pytest

import roi_ref as RR
import stereo_depth_ref as ref
import stereo_ref as SR
import test_stereo_tracker_gpu as ST
from stereo_ref import stamp

pytestmark = pytest.mark.gpu

# The handle's own left camera (gfamd.default_cfg; the oracle's default is the same pinhole) and two right cameras beside it: the thirds of SR.right_frame are
# shifted by 3, 7 and 12 px, which at f = 604 and a 0.05 m baseline are depths of about 10.1, 4.3 and 2.5 m; max_depth 6 sends the first third to `range`.
LEFT = ref.camera("PINHOLE", (603.95556640625, 603.1257934570312, 324.0858154296875, 232.72303771972656))
RIGHT = [ref.camera("PINHOLE", (603.9, 603.2, 324.1, 232.7), (1.0e-3, -2.0e-3, 1.0e-4, -1.0e-4)),
         ref.camera("PINHOLE_FULL", (604.0, 603.1, 324.0, 232.8), (2.0e-3, -1.0e-3, 1.0e-4, 2.0e-4, 5.0e-4, 1.0e-3, -5.0e-4, 1.0e-4))]
RIG = ref.cfg(ref.IDENTITY, (0.05, 0.0, 0.0), 6.0)
A, T = SR.CASES
ZERO = dict(calls=0, launches=0, points=0, with_depth=0, no_match=0, lift=0, parallax=0, behind=0, epipolar=0, range=0)


def _lift(gf, cam):
    if cam["model"] == "PINHOLE":
        return lambda p: SR.pinhole_lift(cam["proj"], cam["dist"], p)
    return lambda p, c=ref.gf(cam): gf.camera_lift([c], [p], rays=False)[0][0]


def _run(gf, oracle, handle_case, seqs, schedule, null_right=(), sizes=False, cap_one_eye=False):
    """seqs[q] = (case, seed, right camera index or None, flow_back, depth): depth None -- no stereo depth; 1 / 0 -- the switch on with that right_obs.  schedule and
    null_right as test_stereo_tracker_gpu._run.  Returns (the bytes every call returned, the depth stats, the tracker's stats, the census by reason)."""
    W, H = handle_case[:2]
    max_cnt, min_dist = max(c[0][2] for c in seqs), min(c[0][3] for c in seqs)
    B = len(seqs)
    g = gf.FeatureTracker(gf.default_cfg(width=W, height=H, batch=B, max_cnt=max_cnt, min_dist=min_dist, flow_back=1, depth_cam=0))
    cap0 = g.cap
    refs, left, right, surf_l, surf_r, cfgs = [], [], [], [], [], []
    for q, (case, seed, cam, fb, sd) in enumerate(seqs):
        w, h, mc, md = case
        if sizes and (w, h) != (W, H):
            g.set_seq_size(q, w, h)
        g.set_seq_cfg(q, max_cnt=mc, min_dist=md, flow_back=fb)
        c = None
        if cam is not None:
            g.set_seq_stereo(q, ref.gf(RIGHT[cam]))
            if sd is not None:
                c = dict(RIG, right_obs=sd)
                g.set_seq_stereo_depth(q, ref.gf_cfg(c))
                assert g.get_seq_stereo_depth(q).as_dict() == ref.gf_cfg(c).as_dict()
        if c is None:
            assert g.get_seq_stereo_depth(q).enable == 0
        cfgs.append(c)
        refs.append(SR.Tracker(oracle, mc, md, fb, _lift(gf, RIGHT[cam]) if cam is not None else None))
        L, R = ST._frames(case, seed)
        left.append(L); right.append(R)
        surf_l.append(ST.Surface(L, False)); surf_r.append(ST.Surface(R, pitched=(q == 0)))
    cap = cap0 if cap_one_eye else g.cap
    if cap_one_eye:
        g.cap = cap0     # an output sized for one eye: enough where no listed sequence emits right observations
    out = np.zeros((B, cap), gf.OBS_DTYPE)
    n_out = np.zeros(B, np.int32)
    frame_of = [0] * B
    want_st = dict(calls=0, launches=0, points=0, matched=0, right_pyramids=0)
    want_sd = dict(ZERO)
    got = []
    for listed in schedule:
        ts, gl, gr, expect = [], [], [], []
        ran = ran_sd = 0
        for q in listed:
            k = frame_of[q]
            frame_of[q] += 1
            stereo = seqs[q][2] is not None
            has_right = stereo and (q, k) not in null_right
            ts.append(stamp(k))
            gl.append(surf_l[q].refs[k])
            gr.append(surf_r[q].refs[k] if has_right else None)
            before = refs[q].census["points"], refs[q].census["kept"]
            ids, cam, obs = refs[q].track(stamp(k), left[q][k], right[q][k] if has_right else None)
            obs = np.array(obs, np.float64)
            if has_right:
                ran += 1
                want_st["points"] += refs[q].census["points"] - before[0]
                want_st["matched"] += refs[q].census["kept"] - before[1]
            if cfgs[q] is not None:
                is_left = cam == 0
                if has_right:       # the restatement on the frame's cur_pts, the right points and the status of the stage
                    cur = refs[q].state()[2]
                    assert len(cur) == int(is_left.sum())
                    rp, st, _, _ = SR.match(oracle, left[q][k], right[q][k], cur, seqs[q][3])
                    mm, why = ref.depth(LEFT, RIGHT[seqs[q][2]], cfgs[q], cur, rp, st)
                    obs[is_left, 7] = mm.astype(np.int32).astype(np.float64) / 1000
                    ran_sd += 1
                    want_sd["points"] += len(cur)
                    cen = ref.census(why)
                    want_sd["with_depth"] += cen["ok"]
                    for name in ("no_match", "lift", "parallax", "behind", "epipolar", "range"):
                        want_sd[name] += cen[name]
                else:
                    obs[is_left, 7] = 0.0
                if not cfgs[q]["right_obs"]:
                    ids, cam, obs = ids[is_left], cam[is_left], obs[is_left]
            expect.append((ids, cam, obs))
        if ran:
            want_st["calls"] += 1; want_st["launches"] += 1; want_st["right_pyramids"] += ran
        if ran_sd:
            want_sd["calls"] += 1; want_sd["launches"] += 1
        n = g.trackImageSomeDeviceRefs(listed, ts, gl, gr if any(r is not None for r in gr) else None, unpack=False, out=out, n_out=n_out)
        for i, q in enumerate(listed):
            ids, cam, obs = expect[i]
            what = "sequence %d, its frame %d" % (q, frame_of[q] - 1)
            assert n[i] == len(ids), "%s: n_out %d, the restatement's %d" % (what, n[i], len(ids))
            o = out[i, :n[i]]
            assert np.array_equal(o["id"], ids) and np.array_equal(o["camera_id"], cam), "%s: ids or camera ids differ" % what
            bad = np.nonzero((o["v"].view(np.uint64) != np.ascontiguousarray(obs).view(np.uint64)).any(axis=1))[0]
            assert len(bad) == 0, "%s: observations %s differ (camera ids %s): %s, the restatement's %s" % (what, bad[:8], cam[bad[:8]], o["v"][bad[:3]], obs[bad[:3]])
            sids, scnt, spts = refs[q].state()
            gids, gcnt, gpts = g.state(q)
            assert np.array_equal(gids, sids) and np.array_equal(gcnt, scnt) and np.array_equal(gpts.view(np.uint32), spts.view(np.uint32)), "%s: state differs" % what
            got.append(o.tobytes())
    assert g.stereo_stats() == want_st, (g.stereo_stats(), want_st)
    sd_stats = g.stereo_depth_stats()
    for q in range(B):
        assert surf_r[q].guards_intact(right[q]), "sequence %d: a right frame or its guard bytes were written" % q
    st = dict(g.stats(), lift=g.camera_lift_stats())
    g.close()
    return got, sd_stats, want_sd, st


FOUR = [(A, 0, 0, 1, 1), (A, 1, 1, 0, 0), (A, 2, 0, 1, None), (A, 3, None, 1, None)]   # depth with right_obs 1, depth with right_obs 0, stereo without depth, mono
THREE = FOUR[:3]
LOCK3, LOCK4 = [[0, 1, 2]] * SR.K, [[0, 1, 2, 3]] * SR.K


def _device(stats, want):
    assert stats == want, (stats, want)
    assert want["with_depth"] > 0 and want["range"] > 0 and want["no_match"] > 0 and want["points"] == sum(want[k] for k in ZERO if k not in ("calls", "launches", "points"))


@pytest.fixture(scope="module")
def lock_step(gf, oracle):
    """the lock-step run of the four sequences on the device form, once: what the variants compare their bytes with"""
    return _run(gf, oracle, A, FOUR, LOCK4)


def test_four_sequences_in_lock_step(lock_step):
    got, stats, want, st = lock_step
    _device(stats, want)
    assert stats["calls"] == SR.K and stats["launches"] == SR.K and stats["points"] == 2 * SR.K * A[2]
    assert 3 * want["with_depth"] >= want["points"] and 6 * want["range"] >= want["points"]     # two thirds of the rows are nearer than max_depth, one third is beyond it


def test_host_form_equals_device_form(gf, oracle, monkeypatch, lock_step):
    monkeypatch.setenv("GF_STEREO_DEPTH_HOST", "1")
    got, stats, want, _ = _run(gf, oracle, A, FOUR, LOCK4)
    assert stats == dict(want, launches=0) and got == lock_step[0]


@pytest.mark.parametrize("lift_host", ["0", "1"])
def test_lift_route_changes_nothing(gf, oracle, monkeypatch, lock_step, lift_host):
    monkeypatch.setenv("GF_CAMERA_LIFT_HOST", lift_host)
    got, stats, want, _ = _run(gf, oracle, A, FOUR, LOCK4)
    _device(stats, want)
    assert got == lock_step[0]


def test_four_points_per_wavefront_in_lk(gf, oracle, monkeypatch, lock_step):
    monkeypatch.setenv("GF_LK_POINTS", "4")
    got, stats, want, _ = _run(gf, oracle, A, FOUR, LOCK4)
    _device(stats, want)
    assert got == lock_step[0]


def test_lists_that_skip_and_reorder_and_a_null_right_entry(gf, oracle):
    schedule = [[2, 0], [1], [0, 1, 2], [1, 0], [0], [2, 1, 0], [1, 2], [0, 1], [2], [2]]
    assert [sum(q in s for s in schedule) for q in range(3)] == [SR.K] * 3
    got, stats, want, _ = _run(gf, oracle, A, THREE, schedule, null_right={(0, 3), (1, 0), (1, 4)})
    _device(stats, want)
    assert stats["calls"] < len(schedule) and stats["points"] == (2 * SR.K - 3) * A[2]       # a null right entry leaves the depth stats as they are


def test_a_frame_size_per_sequence(gf, oracle):
    """132 x 97 and 64 x 61 inside a 188 x 122 handle"""
    M = SR.MIXED
    seqs = [(A, 0, 0, 1, 1), (T, 0, 1, 1, 0), (M, 0, None, 1, None), (T, 1, 0, 0, 1)]
    got, stats, want, _ = _run(gf, oracle, M, seqs, [[0, 1, 2, 3]] * SR.K, sizes=True)
    assert stats == want and stats["launches"] == SR.K and want["with_depth"] > 0


def test_an_output_sized_for_one_eye_suffices_without_right_observations(gf, oracle):
    seqs = [(A, 0, 0, 1, 0), (A, 1, 1, 0, 0)]
    got, stats, want, _ = _run(gf, oracle, A, seqs, [[0, 1]] * 3, cap_one_eye=True)
    assert stats == want and want["with_depth"] > 0
    with pytest.raises(gf.GfError, match="output capacity"):                                   # ... and does not with them
        _run(gf, oracle, A, [(A, 0, 0, 1, 1)], [[0]] * 2, cap_one_eye=True)


def test_a_handle_that_never_calls_the_setter(gf, oracle):
    """stereo sequences without the depth switch: the depth counters stay zero, and the handle launches and lifts what test_stereo_tracker_gpu.py pins for it"""
    seqs = [(A, 0, 0, 1, None), (A, 1, 1, 0, None), (A, 2, None, 1, None)]
    got, stats, want, st = _run(gf, oracle, A, seqs, LOCK3)
    assert stats == ZERO and want == ZERO
    assert st["lift"] == dict(launches=SR.K, sequences=SR.K) and st["lk_launches"] == SR.K - 1
    assert {k: st[k] for k in ST.PYR_COUNTERS} == ST._pyramid_counters(2 * SR.K)


def _snapshot(g, seqs):
    st = g.stats()
    return ([tuple(a.tobytes() for a in g.state(q)) for q in seqs], g.stereo_stats(), g.stereo_depth_stats(), {k: v for k, v in st.items() if not k.startswith("ms_")},
            [g.get_seq_stereo_depth(q).as_dict() for q in seqs])


def test_refusals(gf, oracle):
    """every refusal by name, with state, stats and the configurations as they were"""
    import torch
    w, h, mc, md = A
    g = gf.FeatureTracker(gf.default_cfg(width=w, height=h, batch=3, max_cnt=mc, min_dist=md, flow_back=1, depth_cam=0))
    good = ref.gf_cfg(RIG)

    def refused(match, call):
        before = _snapshot(g, range(3))
        with pytest.raises(gf.GfError, match=match):
            call()
        assert _snapshot(g, range(3)) == before, "a refused call changed state, stats or a configuration (%s)" % match

    refused("gf_tracker_set_seq_stereo", lambda: g.set_seq_stereo_depth(0, good))             # no right camera yet
    refused("sequence 3", lambda: g.set_seq_stereo_depth(3, good))
    g.set_seq_stereo_depth(0, None)                                                            # turning off what is off is accepted
    assert g.stereo_depth_stats() == ZERO
    g.set_seq_stereo(0, ref.gf(RIGHT[0]))
    g.set_seq_stereo(1, ref.gf(RIGHT[1]))
    for word, c in __import__("test_stereo_depth_host").refusals():
        if word != "ok":
            refused(word.replace("[", r"\[").replace("]", r"\]"), lambda: g.set_seq_stereo_depth(0, ref.gf_cfg(c)))
    # a sequence that a staged (prefetched) frame lists: refused until gf_tracker_track_prefetched has consumed it
    left, right = SR.scene(w, h)
    g.set_seq_stereo(2, ref.gf(RIGHT[0]))
    g.prefetchHost([left[0].ctypes.data], seqs=[2])
    refused("listed by a staged frame", lambda: g.set_seq_stereo_depth(2, good))
    assert g.get_seq_stereo_depth(2).enable == 0
    g.trackPrefetched([stamp(0)])
    refused("taken a frame", lambda: g.set_seq_stereo_depth(2, good))
    g.set_seq_stereo_depth(0, good)
    g.set_seq_stereo_depth(1, ref.gf_cfg(dict(RIG, right_obs=0)))
    assert g.get_seq_stereo_depth(0).enable == 1 and g.get_seq_stereo_depth(1).right_obs == 0
    g.set_seq_stereo(1, None)                                                                  # turning stereo off turns the depth off
    assert g.get_seq_stereo_depth(1).enable == 0 and g.get_seq_stereo(1).enable == 0
    left, right = SR.scene(w, h)
    d_l, d_r = torch.from_numpy(np.array(left[0])).cuda(), torch.from_numpy(np.array(right[0])).cuda()
    n = g.trackImageSomeDeviceRefs([0], [stamp(0)], [(d_l.data_ptr(), w)], [(d_r.data_ptr(), w)], unpack=False)
    assert n[0] > mc
    refused("taken a frame", lambda: g.set_seq_stereo_depth(0, None))
    refused("taken a frame", lambda: g.set_seq_stereo_depth(0, good))
    g.reset_stats()
    assert g.stereo_depth_stats() == ZERO
    g.close()
