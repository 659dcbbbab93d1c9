"""Stereo depth behind the tracker: an estimator that owns a stereo-depth tracker (gf_estimator_set_stereo_depth, gf_estimator_input_image_refs) hands its back end
exactly what a stand-alone tracker with the same settings returns, one observation per feature and frame; and a closed loop without images, in which the depth of
every observation comes from gfamd.stereo_depth on noisy pixel pairs of a 0.10 m rig, is held against the same stream fed with the depth image's millimetres.
Run with -m gpu.

Closed loop, measured on the MI355X (stream 1 of test_estimator_gpu.py, 1600 landmarks, 0.2 px noise per eye, 0.971 m driven, 14992 observations with a depth in
either run), position error against the stream's ground truth: RGB-D 0.0027 m at the last frame and 0.0117 m at its worst; stereo depths 0.0028 m and 0.0117 m.
The bar, twice the RGB-D run's error, is met (profiles/stereo_depth_measure.json).  And a group of two estimators fed by one batched stereo-depth tracker with
right_obs 0: each member ends where the same member ends alone."""
import numpy as np
import pytest

import stereo_depth_ref as ref
import stereo_ref as SR
import synth
import synth_stream as SS
import test_stereo_depth_tracker_gpu as TD
import test_stereo_tracker_gpu as ST
from stereo_ref import stamp

pytestmark = pytest.mark.gpu

NON_LINEAR = 1
ORDER = [0, 1, 2, 3, 4, 5, 4, 3]     # eight frames out of the scene's six


def _tracker_cfg(gf, case):
    w, h, mc, md = case
    return gf.default_cfg(width=w, height=h, batch=1, max_cnt=mc, min_dist=md, flow_back=1, depth_cam=0)


def test_estimator_hands_its_back_end_what_a_tracker_returns(gf):
    import torch
    case = TD.A
    w, h, mc, md = case
    left, right = SR.scene(w, h)
    d_l = [torch.from_numpy(np.array(f)).cuda() for f in left]
    d_r = [torch.from_numpy(np.array(f)).cuda() for f in right]
    rig = ref.gf_cfg(TD.RIG)                                              # right_obs 1 as given: the estimator forces 0
    right_cam = ref.gf(TD.RIGHT[1])
    # refusals by name, nothing changed: an estimator whose tracker has a depth camera (one that reads no depth, cfg.depth 0, is refused at its creation already)
    t = _tracker_cfg(gf, case)
    t.depth_cam = 1
    e = gf.SlidingWindowEstimator(gf.default_estimator_cfg(with_tracker=1, multiple_thread=0, use_wheel=0, tracker=t))
    with pytest.raises(gf.GfError, match="depth_cam"):
        e.set_stereo_depth(right_cam, rig)
    e.close()
    e = gf.SlidingWindowEstimator(gf.default_estimator_cfg(with_tracker=0))
    with pytest.raises(gf.GfError, match="without a tracker"):
        e.set_stereo_depth(right_cam, rig)
    with pytest.raises(gf.GfError, match="without a tracker"):
        e.inputImageRefs(0.0, (d_l[0].data_ptr(), w), None)
    e.close()

    est = gf.SlidingWindowEstimator(gf.default_estimator_cfg(with_tracker=1, multiple_thread=0, use_wheel=0, tracker=_tracker_cfg(gf, case)))
    assert est.cfg.depth == 1 and est.cfg.use_imu == 1
    bad = ref.gf_cfg(dict(TD.RIG, max_depth=70.0))
    with pytest.raises(gf.GfError, match="65.535"):                       # the second setter refuses: the first one is taken back
        est.set_stereo_depth(right_cam, bad)
    est.set_stereo_depth(right_cam, rig)
    trk = gf.FeatureTracker(_tracker_cfg(gf, case))
    trk.set_seq_stereo(0, right_cam)
    trk.set_seq_stereo_depth(0, ref.gf_cfg(dict(TD.RIG, right_obs=0)))
    per_frame = []
    with_depth, t_imu, held_any = 0, -0.005, False
    for n_th, k in enumerate(ORDER):
        t = stamp(n_th)
        while t_imu + 0.005 <= t + 0.03:                                  # a platform at rest, 200 Hz: the back end takes a frame once the samples reach it
            t_imu += 0.005
            est.inputIMU(t_imu, (0.0, 0.0, 9.81), (0.0, 0.0, 0.0))
        r1 = (d_r[k].data_ptr(), w) if n_th != 5 else None                # one frame without a right image: every depth 0
        ids, cam, obs = est.inputImageRefs(t, (d_l[k].data_ptr(), w), r1)
        n = trk.trackImageSomeDeviceRefs([0], [t], [(d_l[k].data_ptr(), w)], [r1] if r1 else None, unpack=False)
        o = trk._out[0, :n[0]]
        assert np.array_equal(ids, o["id"]) and np.array_equal(cam, o["camera_id"]) and np.array_equal(obs.view(np.uint64), o["v"].view(np.uint64)), "frame %d" % n_th
        assert not cam.any() and len(set(ids.tolist())) == len(ids) and len(ids) == mc           # one observation per feature
        assert (obs[:, 7] >= 0).all() and ((obs[:, 7] > 0).any() if r1 else not obs[:, 7].any())
        with_depth += int((obs[:, 7] > 0).sum())
        per_frame.append(ids.tolist())
        f = est.features()
        held = dict(zip(f["id"].tolist(), f["n_obs"].tolist()))
        # The window's contents are known here: eight frames do not fill a window of ten, so nothing is marginalised or solved, and the window holds the newest
        # frame_count frames the tracker returned (the count is raised behind each frame while the window fills).  One observation per feature and frame: exactly as many as those frames returned the feature in.
        s = est.state()
        assert s["frame_count"] < est.cfg.window_size

        def counts(m):
            seen = {}
            for frame_ids in per_frame[len(per_frame) - m:] if m else []:
                for i in frame_ids:
                    seen[i] = seen.get(i, 0) + 1
            return seen
        fits = [m for m in range(len(per_frame) + 1) if counts(m) == held]
        print("frame %d: frame_count %d, solver_flag %d, %d features held, the newest %s frames account for them" % (n_th, s["frame_count"], s["solver_flag"], len(held), fits))
        assert fits == [s["frame_count"]] and s["frame_count"] == n_th + 1 and s["solver_flag"] == 0, \
            "frame %d: the feature manager's observations per feature are not those of the window's frames (frame_count %d, fits %s)" % (n_th, s["frame_count"], fits)
        held_any |= len(held) > 0 and max(held.values()) >= 2
    assert held_any and est.state()["frame_count"] >= 4, "the back end never held a feature over two frames: the check above saw nothing"
    assert with_depth > 2 * mc and trk.stereo_depth_stats()["calls"] == len(ORDER) - 1
    est.close(); trk.close()


def _closed_loop(gf, stereo):
    """the stream of test_replay_feature_frames_matches_oracle on the HIP estimator -> (reached NON_LINEAR, distance driven, error at the last frame, worst error
    from NON_LINEAR on, observations with a depth)"""
    st = SS.Stream(1, t_still=1.5, t_move=3.0, v_max=0.4, yaw0=0.0, yaw_turn=-0.6, split_x=1.8, turn_delay=0.8)
    st._lm = st._landmarks(1600)
    st._pn = np.random.default_rng(4001).normal(0, 1.0, (len(st.cam_t), len(st._lm), 2))
    right_noise = np.random.default_rng(4101).normal(0, 1.0, (len(st.cam_t), len(st._lm), 2))
    cam = ref.camera("PINHOLE", (synth.FX, synth.FY, synth.CX, synth.CY))
    rig = ref.gf_cfg(ref.cfg(ref.IDENTITY, (0.10, 0.0, 0.0), 65.0))
    est = gf.SlidingWindowEstimator(gf.default_estimator_cfg(tio=SS.TIO, rio=SS.RIO, multiple_thread=1))
    p0 = st.p_wb(st.cam_t[0])
    tp, last, worst, depths, reached = -1.0, None, 0.0, 0, False
    for k in range(len(st.cam_t)):
        tp = st.feed(est, k, tp)
        if k % 2:
            continue
        frame = st.feature_frame(k)
        if stereo:
            ids = sorted(frame)
            tk = st.cam_t[k]
            Xc = (st._lm[ids] - st.p_wb(tk)) @ st.R_wb(tk)
            Xr = Xc - np.array([0.10, 0.0, 0.0])
            lu = np.array([frame[i][3:5] for i in ids], np.float32)
            ru = np.stack([synth.FX * Xr[:, 0] / Xr[:, 2] + synth.CX + 0.2 * right_noise[k, ids, 0], synth.FY * Xr[:, 1] / Xr[:, 2] + synth.CY + 0.2 * right_noise[k, ids, 1]], 1).astype(np.float32)
            (mm,), (why,) = gf.stereo_depth([ref.gf(cam)], [ref.gf(cam)], [rig], [lu], [ru], [np.ones(len(ids), np.uint8)])
            for i, m in zip(ids, mm):
                frame[i][7] = float(int(m)) / 1000
        depths += sum(1 for v in frame.values() if v[7] > 0)
        est.inputFeature(float(st.cam_t[k]), frame)
        s = est.state()
        if s["solver_flag"] == NON_LINEAR:
            fc, tk = s["frame_count"], st.cam_t[k]
            if not reached:
                # The estimator's world is the stream's turned about z (the initialisation zeroes the yaw of its first pose) and moved: both are fixed ONCE, at the
                # frame that reaches NON_LINEAR, while the platform still stands, from the newest pose against the stream's
                reached = True
                A = s["Rs"][fc] @ st.R_wb(tk).T
                psi = np.arctan2(A[1, 0] - A[0, 1], A[0, 0] + A[1, 1])
                Rz = np.array([[np.cos(psi), -np.sin(psi), 0.0], [np.sin(psi), np.cos(psi), 0.0], [0.0, 0.0, 1.0]])
                origin = s["Ps"][fc] - Rz @ st.p_wb(tk)
                assert np.linalg.norm(st.p_wb(tk) - p0) < 1e-9, "the alignment frame is not in the standstill"
            last = float(np.linalg.norm(s["Ps"][fc] - (Rz @ st.p_wb(tk) + origin)))
            worst = max(worst, last)
    driven = float(np.linalg.norm(est.state()["Ps"][est.state()["frame_count"]]))
    est.close()
    return reached, driven, last, worst, depths


def test_closed_loop_on_stereo_depths_against_the_depth_image(gf):
    """the bar: twice the RGB-D run's position error on the same stream, at the last frame and at its worst.  Inside depth_threshold (3 m) a 0.28 px disparity
    error at f = 604 and b = 0.10 m is 3 cm of depth where the depth image has 1 mm, and those depths are held constant in the solve; the factor is a bar to be
    met or missed, not a prediction."""
    rgbd = _closed_loop(gf, False)
    stereo = _closed_loop(gf, True)
    print("closed loop, position error against the stream's ground truth [m]: RGB-D last %.4f worst %.4f (drove %.3f m, %d depths); stereo last %.4f worst %.4f (drove %.3f m, %d depths)"
          % (rgbd[2], rgbd[3], rgbd[1], rgbd[4], stereo[2], stereo[3], stereo[1], stereo[4]))
    assert rgbd[0] and stereo[0], "a run did not reach NON_LINEAR"
    assert rgbd[1] > 0.5 and stereo[1] > 0.5, "a run did not drive away"
    assert stereo[4] > 0.5 * rgbd[4]
    assert stereo[2] <= 2.0 * rgbd[2] and stereo[3] <= 2.0 * rgbd[3], (rgbd, stereo)


def test_a_group_fed_by_one_batched_stereo_depth_tracker(gf):
    """estimator groups take feature frames, so they need no code: one batched tracker whose two stereo sequences carry the depth of their matches and emit no
    right observations feeds a group of two members (a configuration each), and each member has, frame for frame and bit for bit, the state the same member gets
    as a stand-alone estimator on the same frames"""
    import torch
    case = TD.A
    w, h, mc, md = case
    scenes = [ST._frames(case, seed) for seed in (0, 1)]
    d_l = [[torch.from_numpy(np.array(f)).cuda() for f in L] for L, _ in scenes]
    d_r = [[torch.from_numpy(np.array(f)).cuda() for f in R] for _, R in scenes]
    trk = gf.FeatureTracker(gf.default_cfg(width=w, height=h, batch=2, max_cnt=mc, min_dist=md, flow_back=1, depth_cam=0))
    for q in range(2):
        trk.set_seq_stereo(q, ref.gf(TD.RIGHT[q]))
        trk.set_seq_stereo_depth(q, ref.gf_cfg(dict(TD.RIG, right_obs=0)))
    cfgs = lambda: [gf.default_estimator_cfg(multiple_thread=1, use_wheel=0, wdetect=0, use_mcc=q) for q in range(2)]
    grp = gf.EstimatorGroup(cfgs=cfgs())
    solo = [gf.SlidingWindowEstimator(c) for c in cfgs()]
    out, n_out = np.zeros((2, mc), gf.OBS_DTYPE), np.zeros(2, np.int32)
    trk.cap = mc                                                            # an output sized for one eye suffices without right observations
    t_imu, with_depth = -0.005, 0
    for n_th, k in enumerate(ORDER):
        t = stamp(n_th)
        while t_imu + 0.005 <= t + 0.03:
            t_imu += 0.005
            for e in grp.members + solo:
                e.inputIMU(t_imu, (0.0, 0.0, 9.81), (0.0, 0.0, 0.0))
        null = n_th == 5                                                    # one frame without right images
        n = trk.trackImageSomeDeviceRefs([0, 1], [t, t], [(d_l[q][k].data_ptr(), w) for q in range(2)], None if null else [(d_r[q][k].data_ptr(), w) for q in range(2)],
                                         unpack=False, out=out, n_out=n_out)
        frames = []
        for q in range(2):
            o = out[q, :n[q]]
            assert n[q] == mc and not o["camera_id"].any() and ((o["v"][:, 7] > 0).any() != null)
            with_depth += int((o["v"][:, 7] > 0).sum())
            frames.append({int(i): v.copy() for i, v in zip(o["id"], o["v"])})
        grp.inputFeatures([0, 1], [t, t], frames)
        for q in range(2):
            solo[q].inputFeature(t, frames[q])
            a, b = grp.members[q].state(), solo[q].state()
            for key in ("frame_count", "solver_flag", "marginalization_flag", "n_features", "iterations"):
                assert a[key] == b[key], (n_th, q, key)
            for key in ("Ps", "Rs", "Vs", "Bas", "Bgs", "Headers"):
                assert np.array_equal(np.asarray(a[key]).view(np.uint64), np.asarray(b[key]).view(np.uint64)), (n_th, q, key)
            fa, fb = grp.members[q].features(), solo[q].features()
            for key in fa:
                assert np.array_equal(fa[key], fb[key]) if fa[key].dtype != np.float64 else np.array_equal(fa[key].view(np.uint64), fb[key].view(np.uint64)), (n_th, q, key)
    for q in range(2):
        s, f = grp.members[q].state(), grp.members[q].features()
        assert s["frame_count"] >= 4 and f["id"].size >= mc and f["n_obs"].max() >= 2, "member %d took no frames: the comparison saw nothing" % q
    assert with_depth > 4 * mc and trk.stereo_depth_stats()["launches"] == len(ORDER) - 1
    grp.close(); trk.close()
    for e in solo:
        e.close()
