"""gf_estimator_group_create_each: the members of one estimator group built from a configuration each, on the streams of
tests/test_estimator_gpu.py::test_group_of_sequences_on_one_batched_solver.  Every member has to end up, bit for bit, where a stand-alone
SlidingWindowEstimator with its configuration does on the same inputs, while the solves still leave as one batch -- also with the members' IMU
pre-integrations and per-feature sweeps routed through the group's batched launches, which then carry the members' own noise parameters, depth_threshold,
init_depth and focal_length.  Run with -m gpu."""
import numpy as np
import pytest

import gfamd
import synth_stream as SS

pytestmark = pytest.mark.gpu
N = 4
# what the members differ in: the outlier check, the time offset being estimated, the IMU noise, the depth gate and the wheel's scale
MIXED = [dict(use_mcc=0), dict(use_mcc=1, acc_n=0.2, gyr_n=0.02), dict(use_mcc=0, estimate_td=1, depth_threshold=6.0), dict(use_mcc=1, sx=1.002, acc_n=0.05, gyr_n=0.008)]
# ... and, for the batched launches, in everything else a launch used to take once: the bias random walks, the depth a failed triangulation falls back to and
# the focal length of the outlier check (use_mcc 1 on three members: movingConsistencyCheckW runs for them)
MIXED_MORE = [dict(use_mcc=1), dict(use_mcc=1, acc_n=0.2, gyr_n=0.02, acc_w=0.004, gyr_w=0.0004, init_depth=3.0),
              dict(use_mcc=0, estimate_td=1, depth_threshold=6.0, init_depth=8.0), dict(use_mcc=1, sx=1.002, acc_n=0.05, gyr_n=0.008, focal_length=460.0)]


def _cfg(**kw):
    return gfamd.default_estimator_cfg(tio=SS.TIO, rio=SS.RIO, multiple_thread=1, **kw)


def _streams(t_move=1.6):
    out = []
    for s in range(N):
        st = SS.Stream(1 + s, t_still=1.5, t_move=t_move, v_max=0.4, yaw0=0.0, yaw_turn=-0.4 + 0.2 * s, split_x=1.8, turn_delay=0.6)
        st._lm = st._landmarks(900)
        st._pn = np.random.default_rng(4100 + s).normal(0, 1.0, (len(st.cam_t), len(st._lm), 2))
        out.append(st)
    return out


def _rot_angle(Ra, Rb):
    out = 0.0
    for a, b in zip(Ra, Rb):
        c = (np.trace(a.T @ b) - 1.0) / 2.0
        s = np.linalg.norm(a.T @ b - (a.T @ b).T) / (2.0 * np.sqrt(2.0))
        out = max(out, float(np.arctan2(s, c)))
    return out


def _replay(grp, others, streams):
    """the streams through the group and through others[s] (estimators or the members of a second group, fed by `feed_others`); returns the worst deviation"""
    tp = [-1.0] * N
    nk = min(len(st.cam_t) for st in streams)
    worst = 0.0
    for k in range(nk):
        for s, st in enumerate(streams):
            st.feed(grp.members[s], k, tp[s])
            tp[s] = st.feed(others.members[s] if hasattr(others, "members") else others[s], k, tp[s])
        if k % 2:
            continue
        frames = [st.feature_frame(k) for st in streams]
        ts = [float(st.cam_t[k]) for st in streams]
        grp.inputFeatures(list(range(N)), ts, frames)
        if hasattr(others, "members"):
            others.inputFeatures(list(range(N)), ts, frames)
        for s in range(N):
            o = others.members[s] if hasattr(others, "members") else others[s]
            if not hasattr(others, "members"):
                o.inputFeature(ts[s], frames[s])
            a, b = grp.members[s].state(), o.state()
            assert a["frame_count"] == b["frame_count"] and a["solver_flag"] == b["solver_flag"] and a["marginalization_flag"] == b["marginalization_flag"], (k, s)
            assert a["iterations"] == b["iterations"] and a["successful_steps"] == b["successful_steps"], (k, s)
            assert list(grp.members[s].features()["id"]) == list(o.features()["id"]), (k, s)
            worst = max(worst, float(np.abs(a["Ps"] - b["Ps"]).max()), _rot_angle(a["Rs"], b["Rs"]))
    return worst


@pytest.mark.parametrize("device_preint,device_sweeps,mixed", [(False, False, MIXED), (True, False, MIXED), (False, True, MIXED), (False, True, MIXED_MORE), (True, True, MIXED_MORE)],
                         ids=["host_loops", "device_preint", "device_sweeps", "device_sweeps_more_fields", "device_both_more_fields"])
def test_members_with_a_configuration_each_on_the_batched_launches(device_preint, device_sweeps, mixed):
    """the group's own launches of the members' pre-integrations (one job per IMU interval) and feature sweeps (one table row per window): every member still is
    the stand-alone estimator of its cfg, which runs both on its host loops"""
    streams = _streams()
    grp = gfamd.EstimatorGroup(cfgs=[_cfg(**kw) for kw in mixed], device_preint=device_preint, device_sweeps=device_sweeps)
    solo = [gfamd.SlidingWindowEstimator(_cfg(**kw)) for kw in mixed]
    worst = _replay(grp, solo, streams)
    st = grp.stats()
    print("mixed group of %d (device_preint %s, device_sweeps %s): worst deviation from stand-alone estimators %.2e; %s" % (N, device_preint, device_sweeps, worst, st))
    assert all(m.state()["solver_flag"] == 1 for m in grp.members)
    assert worst == 0.0
    assert st["largest_batch"] == N
    grp.close()
    for e in solo:
        e.close()


def test_members_with_a_configuration_each():
    streams = _streams()
    cfgs = [_cfg(**kw) for kw in MIXED]
    grp = gfamd.EstimatorGroup(cfgs=cfgs)
    solo = [gfamd.SlidingWindowEstimator(_cfg(**kw)) for kw in MIXED]
    worst = _replay(grp, solo, streams)
    st = grp.stats()
    print("mixed group of %d: worst deviation from stand-alone estimators %.2e; %s" % (N, worst, st))
    assert all(m.state()["solver_flag"] == 1 for m in grp.members)
    assert worst == 0.0
    assert st["largest_batch"] == N
    finals = [m.state()["Ps"].copy() for m in grp.members]
    grp.close()
    for e in solo:
        e.close()
    # the configurations are told apart by the stand-alone estimators themselves: member s with member 0's configuration ends somewhere else
    plain = gfamd.SlidingWindowEstimator(_cfg(**MIXED[0]))
    tp = -1.0
    for k in range(min(len(st.cam_t) for st in streams)):
        tp = streams[1].feed(plain, k, tp)
        if k % 2 == 0:
            plain.inputFeature(float(streams[1].cam_t[k]), streams[1].feature_frame(k))
    assert not np.array_equal(plain.state()["Ps"], finals[1])
    plain.close()


def test_one_configuration_four_times_is_the_plain_group():
    """gf_estimator_group_create(c, 4) and gf_estimator_group_create_each with four copies of c: the same bits"""
    streams = _streams(t_move=0.8)
    cfg = _cfg(use_mcc=1)
    a = gfamd.EstimatorGroup(cfg, N)
    b = gfamd.EstimatorGroup(cfgs=[_cfg(use_mcc=1) for _ in range(N)])
    worst = _replay(a, b, streams)
    for s in range(N):
        x, y = a.members[s].state(), b.members[s].state()
        for key in ("Ps", "Rs", "Vs", "Bas", "Bgs"):
            assert np.array_equal(np.asarray(x[key]).view(np.uint64), np.asarray(y[key]).view(np.uint64)), (s, key)
    assert worst == 0.0 and a.stats() == b.stats()
    a.close(); b.close()


@pytest.mark.parametrize("field,value", [("window_size", 8), ("gnss_enable", 1), ("num_iterations", 4), ("use_imu", 0), ("use_wheel", 0), ("depth", 0)])
def test_members_that_do_not_fit_one_solver_are_refused(field, value):
    cfgs = [_cfg() for _ in range(3)]
    setattr(cfgs[2], field, value)
    with pytest.raises(gfamd.GfError, match="gf status -1.*member 2: %s %d differs from member 0's" % (field, value)):
        gfamd.EstimatorGroup(cfgs=cfgs)


def test_other_refusals():
    cfgs = [_cfg() for _ in range(3)]
    cfgs[1].with_tracker = 1
    with pytest.raises(gfamd.GfError, match="gf status -1.*member 1: .*with_tracker"):
        gfamd.EstimatorGroup(cfgs=cfgs)
    cfgs = [_cfg() for _ in range(3)]
    cfgs[2].max_solver_time = 0.04
    with pytest.raises(gfamd.GfError, match="gf status -1.*member 2: max_solver_time"):
        gfamd.EstimatorGroup(cfgs=cfgs)
    with pytest.raises(gfamd.GfError, match="gf status -1"):
        gfamd.EstimatorGroup(cfgs=[])
    with pytest.raises(TypeError):
        gfamd.EstimatorGroup(_cfg(), 2, cfgs=[_cfg(), _cfg()])
    g = gfamd.EstimatorGroup(cfgs=[_cfg(max_features=256, max_visual=2048), _cfg()])      # capacities may differ: the shared handle takes the largest
    assert g.n == 2 and g.members[0].cfg.max_features == 256
    g.close()
