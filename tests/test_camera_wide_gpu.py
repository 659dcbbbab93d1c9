"""PINHOLE_FULL and SCARAMUZZA cameras on the device: camera_lift_kernel through gf_camera_lift_batch_ex / _device_ex against the numpy float64 route of
tests/golden/camera_models_wide.json.gz -- bit for bit: neither lift involves a transcendental -- and a tracker handle whose sequences have a PINHOLE_FULL, a
SCARAMUZZA, a KANNALA_BRANDT and a PINHOLE camera against an all-PINHOLE handle on the same frames.  In the tracker tests the expected pairs are the generator's
numpy route (tests/golden/make_camera_wide_golden.py, F = np.float64) on the pixels the tracker reports, and the velocities are recomputed from the reported pairs
as ptsVelocity computes them (feature_tracker.cpp:810-847).  The shared kernel shipped: a call's lift is ONE launch whatever the mix of models, counted by
gf_tracker_get_camera_lift_stats and held call by call against a handle whose non-pinhole sequences are all KANNALA_BRANDT.  By default SCARAMUZZA sequences are
lifted on the host (it measured faster there), so such a sequence is not listed for the kernel; GF_CAMERA_LIFT_HOST=0 / 1 puts every model on the device / the
host, and the comparison runs in all three modes.  Run with -m gpu."""
import ctypes as C
import gzip
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "ground-fusion_amd")):      # also where the module runs as a child process
    if _p not in sys.path:
        sys.path.insert(0, _p)
import synth  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "camera_models_wide.json.gz")
FX = float.fromhex
DT = 0.0666
W, H, K = 176, 192, 6      # the smallest frame with four pyramid levels
HANDLE = dict(max_cnt=40, min_dist=12, flow_back=1, depth_cam=1)
FULL = dict(proj=[150.5, 151.25, 88.5, 96.25], dist=[0.52, -2.7, 4e-4, -1.5e-4, 1.5, 0.4, -2.5, 1.4])
# an equidistant fisheye of 60 px per radian and its inverse polynomial (fisheye_polys(60, 140) of the generator): projecting a lifted pixel lands within 0.05 px
SCA = dict(poly=[-58.55429459714, -0.2571091786983, 0.01628196515412, -0.0001582655624318, 8.875057760037e-07],
           inv_poly=[94.64768221243, 59.858579044, -5.311910432481, -0.2540722630341, 11.62947621815, 2.267207606402, -8.244986264687, 0.03464128742445, 5.419260019102,
                     1.417284429096, -0.876101205289, -0.3399781929985], affine=[1.0005, 2e-4, -3e-4, 88.5, 95.25])
KB = ("KANNALA_BRANDT", [80.5, 81.25, 88.5, 96.25], [-0.012, 0.006, -0.003, 0.0006])
LISTS = [[0, 1, 2, 3], [3, 1], [2, 0, 1], [1, 3, 0, 2], [0, 2, 3], [3, 2, 1, 0], [0, 1, 3], [2, 3, 0, 1], [2], [1, 0, 2, 3]]      # skip and reorder; every sequence takes > K frames' worth
_G = {}


def _gen():
    """the generator's transcriptions (numpy float64 route), without its global mpmath precision"""
    if "g" not in _G:
        import mpmath
        import make_camera_wide_golden as g
        mpmath.mp.dps = 15
        _G["g"] = g
    return _G["g"]


def _fixture():
    if "doc" not in _G:
        _G["doc"] = json.loads(gzip.open(GOLDEN).read())
    return _G["doc"]


def _same(got, want, what):
    """the bits where `want` is finite, not finite where it is not"""
    got, want = np.asarray(got), np.asarray(want, got.dtype)
    ok = np.isfinite(want)
    view = np.uint64 if got.dtype == np.float64 else np.uint32
    assert np.array_equal(got[ok].view(view), want[ok].view(view)), "%s: %d finite values differ in their bits" % (what, int((got[ok].view(view) != want[ok].view(view)).sum()))
    assert not np.isfinite(got[~ok]).any(), what + ": a finite value where the reference's double route has none"


def _numpy_pairs(kind, cam, uv):
    """the float pairs of the reference's double route on float pixels"""
    g = _gen()
    out = np.zeros((len(uv), 2), np.float32)
    with np.errstate(all="ignore"):
        for i, (u, v) in enumerate(np.asarray(uv, np.float64)):
            P = g.full_lift(cam["proj"], cam["dist"], float(u), float(v), np.float64)[0] if kind == 3 else g.sca_lift(cam["poly"], cam["affine"], float(u), float(v), np.float64, np.sqrt)[0]
            out[i] = (np.float32(P[0] / P[2]), np.float32(P[1] / P[2]))
    return out


def _batch(gf):
    """all five models in one batch, 0, 1, 63, 64, 65 and 129 points per entry; neighbours differ in their model; models 3 and 4 each see every count"""
    if "batch" in _G:
        return _G["batch"]
    doc = _fixture()
    by = {c["name"]: c for c in doc["cases"]}
    ex = gf.CameraModelEx
    old = {"PINHOLE": gf.CameraModel.make("PINHOLE", [603.95556640625, 603.1257934570312, 324.0858154296875, 232.72303771972656], [0.148, -0.468, 1.6e-3, -8.9e-3]),
           "MEI": gf.CameraModel.make("MEI", [470.5, 468.25, 320.5, 240.25], [-0.02, 0.003, 2e-4, -1e-4], 1.0),
           "KB": gf.CameraModel.make("KANNALA_BRANDT", [285.5, 286.25, 320.5, 240.25], [-0.9, 0.35, -0.05, 0.0025])}
    order = [("full_kinect8", 129), ("sca_affine", 0), ("PINHOLE", 64), ("full_pole", 1), ("sca_190_identity", 63), ("MEI", 129), ("full_barrel", 64), ("sca_horizon_inside", 65),
             ("KB", 63), ("full_opencv5", 65), ("sca_affine", 129), ("full_zero", 0), ("KB", 1), ("sca_190_identity", 64), ("full_kinect8", 63), ("MEI", 65), ("sca_horizon_inside", 1),
             ("PINHOLE", 0)]
    rng = np.random.default_rng(11)
    cams, pts, exp = [], [], []
    for name, n in order:
        if name in old:
            cams.append(old[name])
            pts.append(np.stack([rng.uniform(0, 639, n), rng.uniform(0, 479, n)], 1).astype(np.float32))
            exp.append(None)      # the old call's bits
            continue
        c = by[name]
        cams.append(ex.make(c["model"], c.get("proj", [0] * 4), c.get("dist", ()), 0.0, c.get("poly", ()), c.get("inv_poly", ()), c.get("affine", ())))
        idx = np.arange(n) % len(c["points"])      # the NaN and infinite pixels among them: they share wavefronts with finite ones
        pts.append(np.array([[FX(t) for t in c["points"][i]["uv"]] for i in idx], np.float32).reshape(n, 2))
        exp.append((np.array([[FX(t) for t in c["points"][i]["ray_d"]] for i in idx]).reshape(n, 3), np.array([[FX(t) for t in c["points"][i]["un_d"]] for i in idx], np.float32).reshape(n, 2)))
    assert all(a.model != b.model for a, b in zip(cams, cams[1:])) and {c.model for c in cams} == {0, 1, 2, 3, 4}
    for model in (3, 4):
        assert {len(p) for c, p in zip(cams, pts) if c.model == model} == {0, 1, 63, 64, 65, 129}
    _G["batch"] = (cams, pts, exp)
    return _G["batch"]


def _check_batch(gf, cams, pts, exp, un, rays, what):
    for b in range(len(cams)):
        assert un[b].shape == (len(pts[b]), 2) and (rays is None or rays[b].shape == (len(pts[b]), 3))
        if not len(pts[b]):
            continue
        w = "%s, entry %d (model %d, %d points)" % (what, b, cams[b].model, len(pts[b]))
        if exp[b] is None:
            o_un, o_rays = gf.camera_lift([cams[b]], [pts[b]])      # gf_camera_lift_batch
            assert un[b].tobytes() == o_un[0].tobytes() and (rays is None or rays[b].tobytes() == o_rays[0].tobytes()), w + ": not the bits of gf_camera_lift_batch"
        else:
            _same(un[b], exp[b][1], w + ", pairs")
            if rays is not None:
                _same(rays[b], exp[b][0], w + ", rays")


# ---- 1: the lift as a building block
def test_lift_batch_gives_the_bits_of_the_double_route(gf):
    cams, pts, exp = _batch(gf)
    un, rays = gf.camera_lift(cams, pts)
    _check_batch(gf, cams, pts, exp, un, rays, "host arrays")
    un2, none = gf.camera_lift(cams, pts, rays=False)      # the kernel writes no rays: the pairs keep their bits
    assert none is None and all(a.tobytes() == b.tobytes() for a, b in zip(un, un2))
    for q in range(len(cams)):      # each entry alone, as behind a longer batch
        if len(pts[q]):
            a_un, a_rays = gf.camera_lift([gf.CameraModelEx.of(cams[q])], [pts[q]])
            assert a_un[0].tobytes() == un[q].tobytes() and a_rays[0].tobytes() == rays[q].tobytes(), "entry %d alone" % q


def test_lift_batch_on_device_arrays(gf):
    import torch
    cams, pts, exp = _batch(gf)
    flat = np.concatenate(pts)
    n = len(flat)
    first = np.concatenate([[0], np.cumsum([len(p) for p in pts])])
    d_uv = torch.from_numpy(flat).cuda()
    d_un = torch.full((n + 8, 2), -7.0, dtype=torch.float32, device="cuda")
    d_rays = torch.full((n + 8, 3), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    gf.camera_lift_device(cams, [len(p) for p in pts], d_uv.data_ptr(), d_rays.data_ptr(), d_un.data_ptr(), stream=s.cuda_stream)
    un, rays = d_un.cpu().numpy(), d_rays.cpu().numpy()
    assert (un[n:] == -7.0).all() and (rays[n:] == -7.0).all()      # nothing behind the last point
    cut = lambda a: [a[first[b]:first[b + 1]] for b in range(len(cams))]
    _check_batch(gf, cams, pts, exp, cut(un), cut(rays), "device arrays")
    d_un.fill_(-7.0)
    torch.cuda.synchronize()
    gf.camera_lift_device(cams, [len(p) for p in pts], d_uv.data_ptr(), None, d_un.data_ptr())      # no rays, the null stream
    assert d_un.cpu().numpy().tobytes() == un.tobytes()


# ---- 2: the tracker
def _frames():
    if "frames" not in _G:
        _G["frames"] = ([synth.tracker_sequence(s, len(LISTS), W, H) for s in (3100, 3101, 3102, 3103)], np.full((H, W), 1500, np.uint16))
    return _G["frames"]


def _cameras(gf):
    return [gf.CameraModelEx.make("PINHOLE_FULL", **FULL), gf.CameraModelEx.make("SCARAMUZZA", **SCA), gf.CameraModel.make(*KB), None]


def _velocities(ids, un, prev, dt):
    """ptsVelocity (feature_tracker.cpp:810-847) on reported float pairs: prev = {id: pair} of the frame before, or None on the first frame"""
    v = np.zeros((len(ids), 2), np.float32)
    for i, fid in enumerate(ids):
        if prev is not None and int(fid) in prev:
            d = un[i] - prev[int(fid)]                                   # float - float
            v[i] = (d.astype(np.float64) / np.float64(dt)).astype(np.float32)
    return v


def _counters(t):
    return {k: v for k, v in t.stats().items() if not k.startswith("ms_")}


def _mixed_against_pinholes(gf, mode=None):
    """mode: GF_CAMERA_LIFT_HOST of this process -- None (unset: SCARAMUZZA on the host, the other models on the device), "0" (all on the device), "1" (all on
    the host).  kbs: the same handle with KANNALA_BRANDT in the place of PINHOLE_FULL and SCARAMUZZA"""
    assert os.environ.get("GF_CAMERA_LIFT_HOST") == mode
    frames, depth = _frames()
    cams = _cameras(gf)
    mixed, plain, kbs = [gf.FeatureTracker(gf.default_cfg(width=W, height=H, batch=4, **HANDLE)) for _ in range(3)]
    for b in range(3):
        mixed.set_seq_camera(b, cams[b])
        kbs.set_seq_camera(b, cams[2])
    on_device = {None: {0, 2}, "0": {0, 1, 2}, "1": set()}[mode]      # the sequences of `mixed` that the kernel lifts
    kb_device = set() if mode == "1" else {0, 1, 2}
    lifts = {"mixed": 0, "kbs": 0}
    assert mixed.get_seq_camera(0, gf.CameraModelEx).as_dict() == cams[0].as_dict() and mixed.get_seq_camera(1, gf.CameraModelEx).as_dict() == cams[1].as_dict()
    assert mixed.get_seq_camera(2).as_dict() == cams[2].as_dict() and mixed.get_seq_camera(2, gf.CameraModelEx).as_dict() == gf.CameraModelEx.of(cams[2]).as_dict()
    for b, word in ((0, "PINHOLE_FULL"), (1, "SCARAMUZZA")):      # the 80-byte struct cannot carry them
        with pytest.raises(gf.GfError, match=word + ".*gf_tracker_get_seq_camera_ex"):
            mixed.get_seq_camera(b)
    nxt, prev, last_t, carried = [0] * 4, [None] * 4, [0.0] * 4, 0
    for L in LISTS:
        ts = [DT * nxt[b] + 0.001 * b for b in L]
        imgs = [frames[b][nxt[b]] for b in L]
        res = mixed.trackImageSome(L, ts, imgs, [depth] * len(L))
        ref = plain.trackImageSome(L, ts, imgs, [depth] * len(L))
        kbs.trackImageSome(L, ts, imgs, [depth] * len(L))
        # ONE launch for a call that lists a sequence lifted on the device, whatever the models among them, none otherwise: the KANNALA_BRANDT handle's count
        for name, t, dev in (("mixed", mixed, on_device), ("kbs", kbs, kb_device)):
            got = t.camera_lift_stats()["launches"]
            assert got - lifts[name] == (1 if dev & set(L) else 0), "%s, list %s: %d lift launches in one call" % (name, L, got - lifts[name])
            lifts[name] = got
        assert plain.camera_lift_stats() == {"launches": 0, "sequences": 0}
        for i, b in enumerate(L):
            (ids, obs), (pid, pobs) = res[i], ref[i]
            what = "frame %d of sequence %d" % (nxt[b], b)
            assert np.array_equal(ids, pid), what + ": ids differ from the pinhole handle's"
            assert np.array_equal(obs[:, [2, 3, 4, 7]].view(np.uint64), pobs[:, [2, 3, 4, 7]].view(np.uint64)), what + ": pixel coordinates or depths differ"
            assert all(np.array_equal(x, y) for x, y in zip(mixed.state(b), plain.state(b))), what + ": ids / track counts / points of the state differ"
            if b == 3:
                assert np.array_equal(obs.view(np.uint64), pobs.view(np.uint64)), what + ": the pinhole sequence's output differs"
            else:
                assert (obs[:, 0:2] == obs[:, 0:2].astype(np.float32)).all() and (obs[:, 5:7] == obs[:, 5:7].astype(np.float32)).all()
                un = obs[:, 0:2].astype(np.float32)
                if b < 2:      # the numpy route of the reference on the reported pixels, bit for bit
                    _same(un, _numpy_pairs(3 + b, FULL if b == 0 else SCA, obs[:, 3:5]), what + ": lifted pairs")
                    assert np.isfinite(un).all()
                else:
                    blk = gf.camera_lift([cams[2]], [obs[:, 3:5]], rays=False)[0][0]
                    assert np.array_equal(un.view(np.uint32), blk.view(np.uint32)), what
                want = _velocities(ids, un, prev[b], ts[i] - last_t[b])
                assert np.array_equal(obs[:, 5:7].astype(np.float32).view(np.uint32), want.view(np.uint32)), what + ": velocities are not ptsVelocity of the lifted pairs"
                carried += 0 if prev[b] is None else sum(1 for f in ids if int(f) in prev[b])
                prev[b] = {int(f): un[j] for j, f in enumerate(ids)}
            last_t[b] = ts[i]
            nxt[b] += 1
    assert min(nxt) >= K and carried > 3 * HANDLE["max_cnt"], "too few features were carried from frame to frame for the row index to matter"
    # lk_launches and every other counter: those of the KANNALA_BRANDT handle and of the all-PINHOLE one; the lift's own: launches as counted call by call above
    cm, ck, cp = _counters(mixed), _counters(kbs), _counters(plain)
    assert cm == ck and cm == cp and cm["lk_launches"] > 0 and cm["sequence_frames"] == sum(len(L) for L in LISTS)
    lm, lk = mixed.camera_lift_stats(), kbs.camera_lift_stats()
    assert lm == {"launches": sum(1 for L in LISTS if on_device & set(L)), "sequences": sum(len(on_device & set(L)) for L in LISTS)}
    assert lk == {"launches": sum(1 for L in LISTS if kb_device & set(L)), "sequences": sum(len(kb_device & set(L)) for L in LISTS)}
    if mode == "0":
        assert lm == lk and lm["launches"] > 0      # every model on the device: the KANNALA_BRANDT handle's launches, call by call and in all
    if mode is None:
        assert 0 < lm["launches"] < lk["launches"]  # [3, 1] lists a PINHOLE and a SCARAMUZZA sequence: no launch at all
    mixed.reset_stats()
    assert mixed.camera_lift_stats() == {"launches": 0, "sequences": 0}
    for t in (mixed, plain, kbs):
        t.close()
    return cm


def test_tracker_with_four_models(gf):
    _mixed_against_pinholes(gf, os.environ.get("GF_CAMERA_LIFT_HOST"))


@pytest.mark.parametrize("host", ["1", "0"])
def test_tracker_with_the_lift_switched(host):
    """GF_CAMERA_LIFT_HOST is read when the tracker is created: a fresh child process runs the same comparison with every model lifted on the host (1: no
    launch at all) and on the device (0: SCARAMUZZA too, in the one launch)"""
    env = dict(os.environ, GF_CAMERA_LIFT_HOST=host)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--host-lift-child"], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0 and "lift switched: ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


# ---- 3: the identity
def test_pinhole_full_without_distortion_is_the_pinhole(gf, tmp_path):
    """both are (1 / f) u - c / f: the same bits from the kernel, in all eight fields of every observation through the tracker, in the vio.txt gf_replay
    writes on a short synthetic recording, and in the observations and the window of an estimator given the camera"""
    frames, depth = _frames()
    cfg = gf.default_cfg(width=W, height=H, batch=1, **HANDLE)
    proj = [cfg.fx, cfg.fy, cfg.cx, cfg.cy]
    full0, pin0 = gf.CameraModelEx.make("PINHOLE_FULL", proj), gf.CameraModel.make("PINHOLE", proj)
    rng = np.random.default_rng(4)
    uv = np.stack([rng.uniform(-50, 700, 257), rng.uniform(-50, 530, 257)], 1).astype(np.float32)
    a, b = gf.camera_lift([full0], [uv]), gf.camera_lift([pin0], [uv])
    assert a[0][0].tobytes() == b[0][0].tobytes() and a[1][0].tobytes() == b[1][0].tobytes()
    ta, tb = gf.FeatureTracker(cfg), gf.FeatureTracker(cfg)
    ta.set_seq_camera(0, full0)
    for k in range(4):
        (ia, oa), (ib, ob) = ta.trackImage(DT * k, frames[0][k], depth), tb.trackImage(DT * k, frames[0][k], depth)
        assert np.array_equal(ia, ib) and np.array_equal(oa.view(np.uint64), ob.view(np.uint64)) and len(ia) > 10, "frame %d" % k
    ta.close(); tb.close()

    import synth_stream as SS
    st = SS.Stream(1, t_still=1.5, t_move=1.0, v_max=0.4, yaw0=0.0, yaw_turn=-0.6, split_x=1.8, turn_delay=0.8)
    d = str(tmp_path)
    n = st.export(d)
    cfg_path = os.path.join(d, "config.yaml")
    t = gf.estimator_cfg_from_yaml(cfg_path).tracker
    calib = os.path.join(d, [l.split(":", 1)[1].strip().strip('"') for l in open(cfg_path) if l.startswith("cam0_calib")][0])
    body = "camera_name: camera\nimage_width: %d\nimage_height: %d\ndistortion_parameters:\n   k1: 0.0\n   k2: 0.0\n   p1: 0.0\n   p2: 0.0\nprojection_parameters:\n   fx: %r\n   fy: %r\n   cx: %r\n   cy: %r\n" % (
        t.width, t.height, t.fx, t.fy, t.cx, t.cy)
    exe = os.path.join(ROOT, "bin", "gf_replay")
    vio = {}
    for name in ("PINHOLE", "PINHOLE_FULL"):
        open(calib, "w").write("%YAML:1.0\n---\nmodel_type: " + name + "\n" + body)
        out = subprocess.run([exe, cfg_path, d, os.path.join(d, name + ".txt")], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0 and "%d RGB-D pairs (0 / 0 unpaired" % n in out.stdout, out.stderr
        vio[name] = open(os.path.join(d, name + ".txt"), "rb").read()
        ecfg, cam = gf.estimator_cfg_from_yaml_camera_ex(cfg_path)      # an estimator of this process given the camera: its observations and its window
        assert cam.model == (0 if name == "PINHOLE" else 3)
        est = gf.SlidingWindowEstimator(ecfg)
        if cam.model:
            est.set_camera(cam)
        seen = []
        for k in range(min(n, 15)):
            gray, dep = st.image(k)
            obs = est.inputImage(float(st.cam_t[k]), gray, dep)
            seen.append(b"".join(np.int64(i).tobytes() + obs[i].tobytes() for i in sorted(obs)))
        state = est.state()
        vio["est_" + name] = b"".join(seen) + state["Ps"].tobytes() + state["Rs"].tobytes()
        assert len(seen[-1]) > 10 * 72      # more than ten observations of id and eight doubles in the last frame
        if cam.model:
            with pytest.raises(gf.GfError, match="has taken a frame"):
                est.set_camera(cam)
        est.close()
    assert len(vio["PINHOLE"].splitlines()) > 5 and vio["PINHOLE"] == vio["PINHOLE_FULL"], "gf_replay: the vio.txt of the PINHOLE_FULL file is not the PINHOLE file's"
    assert vio["est_PINHOLE"] == vio["est_PINHOLE_FULL"], "the estimator given the PINHOLE_FULL camera differs from the PINHOLE one"


# ---- 4: prediction
@pytest.mark.parametrize("model", [3, 4])
def test_set_prediction_goes_through_the_model(gf, model):
    """predictions for the sequence are points whose projection gf_camera_project_batch_ex gives; a pinhole handle gets points that project to the same float
    pixels: the next frame is the same, bit for bit, in everything that does not depend on the model, so LK started where the projection says"""
    frames, depth = _frames()
    cam = _cameras(gf)[model - 3]
    a, b = [gf.FeatureTracker(gf.default_cfg(width=W, height=H, batch=1, **HANDLE)) for _ in range(2)]
    a.set_seq_camera(0, cam)
    par = b.get_seq_cfg(0)
    rng = np.random.default_rng(3)
    moved = 0
    for k in range(4):
        ia, oa = a.trackImage(DT * k, frames[2][k], depth)
        ib, ob = b.trackImage(DT * k, frames[2][k], depth)
        assert np.array_equal(ia, ib) and np.array_equal(oa[:, [2, 3, 4, 7]].view(np.uint64), ob[:, [2, 3, 4, 7]].view(np.uint64)), "frame %d" % k
        assert all(np.array_equal(x, y) for x, y in zip(a.state(), b.state()))
        ids, _, pts = a.state()
        sel = rng.random(len(ids)) < 0.7
        near = (pts[sel] + rng.normal(0, 1.0, (int(sel.sum()), 2))).astype(np.float32)
        xyz = gf.camera_lift([cam], [near])[1][0] * 3.0      # any point on the ray of a pixel near the feature
        target = gf.camera_project([cam], [xyz])[0].astype(np.float32)      # where gf_camera_project_batch_ex puts it: (float)u, (float)v of setPrediction
        assert np.isfinite(target).all() and np.abs(target - near).max() < 2.0
        moved += int((target != pts[sel]).any(axis=1).sum())
        t64 = target.astype(np.float64)
        pxyz = np.stack([(t64[:, 0] - par["cx"]) / par["fx"] * 2.0, (t64[:, 1] - par["cy"]) / par["fy"] * 2.0, np.full(len(t64), 2.0)], 1)
        assert np.array_equal(gf.camera_project([b.get_seq_camera(0)], [pxyz])[0].astype(np.float32), target)
        a.setPrediction(ids[sel], xyz, seq=0)
        b.setPrediction(ids[sel], pxyz, seq=0)
    assert a.stats()["lk_launches"] == b.stats()["lk_launches"] and len(ia) > 10 and moved > 20
    a.close(); b.close()


# ---- 5: refusals on the device path
def test_setter_rules(gf):
    import torch
    frames, depth = _frames()
    lib = gf.lib()
    full, sca, kb, _ = _cameras(gf)
    t = gf.FeatureTracker(gf.default_cfg(width=W, height=H, batch=3, **HANDLE))
    assert lib.gf_tracker_set_seq_camera_ex(None, 0, C.byref(full)) == -1 and lib.gf_tracker_get_seq_camera_ex(None, 0, C.byref(full)) == -1
    for seq in (-1, 3):
        with pytest.raises(gf.GfError, match="gf status -1.*sequence %d of a handle of 3" % seq):
            t.set_seq_camera(seq, full)
    bad_fx = gf.CameraModelEx.make("PINHOLE_FULL", [0.0, 151.25, 88.5, 96.25], FULL["dist"])
    bad_k5 = gf.CameraModelEx.make("PINHOLE_FULL", FULL["proj"], FULL["dist"][:6] + [math.nan])
    bad_aff = gf.CameraModelEx.make("SCARAMUZZA", poly=SCA["poly"], inv_poly=SCA["inv_poly"], affine=[0.5, 2.0, 0.25, 88.5, 95.25])
    for field, bad in (("fx", bad_fx), ("k5", bad_k5), (r"ac - ad \* ae", bad_aff), ("model", gf.CameraModelEx.make(5)), ("model", gf.CameraModel.make(3, FULL["proj"]))):
        with pytest.raises(gf.GfError, match="gf status -1.*sequence 1.*%s" % field):
            t.set_seq_camera(1, bad)
    t.set_seq_camera(0, full)
    t.set_seq_camera(1, sca)
    # a registration: onto PINHOLE and PINHOLE_FULL alone, both ways
    reg = gf.DepthReg.make(W, H, *FULL["proj"])
    t.set_seq_depth_reg(0, reg)
    t.set_seq_depth_reg(2, reg)
    with pytest.raises(gf.GfError, match="sequence 1 has a SCARAMUZZA camera"):
        t.set_seq_depth_reg(1, reg)
    with pytest.raises(gf.GfError, match="sequence 0 has a depth registration.*SCARAMUZZA"):
        t.set_seq_camera(0, sca)
    with pytest.raises(gf.GfError, match="sequence 2 has a depth registration.*KANNALA_BRANDT"):
        t.set_seq_camera(2, kb)
    t.set_seq_camera(2, full)      # PINHOLE_FULL while a registration is set
    t.set_seq_camera(0, full)
    t.set_seq_depth_reg(0, None)
    t.set_seq_depth_reg(2, None)
    # after a frame, and while a frame is staged
    t.trackImageSome([1], [0.0], [frames[0][0]], [depth])
    with pytest.raises(gf.GfError, match="gf status -1.*sequence 1 has taken a frame"):
        t.set_seq_camera(1, full)
    assert t.get_seq_camera(1, gf.CameraModelEx).as_dict() == sca.as_dict()
    t.reset_seq(1)
    assert t.get_seq_camera(1, gf.CameraModelEx).as_dict() == sca.as_dict()      # a setting: kept by the reset, and settable again
    t.set_seq_camera(1, full)
    g = torch.from_numpy(np.ascontiguousarray(frames[0][0])).pin_memory()
    d = torch.from_numpy(depth.view(np.int16)).pin_memory()
    t.prefetchHost([g.data_ptr()], [d.data_ptr()], seqs=[1])
    with pytest.raises(gf.GfError, match="gf status -1.*sequence 1 is listed by a staged frame"):
        t.set_seq_camera(1, sca)
    t.trackPrefetched([0.0])
    assert t.get_seq_camera(1, gf.CameraModelEx).as_dict() == full.as_dict()
    # back to a pinhole through the wide setter: the eight fields of the sequence's parameters, and the old getter answers again
    t.reset_seq(1)
    t.set_seq_camera(1, gf.CameraModelEx.make("PINHOLE", [150.5, 151.5, 88.0, 96.0], [0.1, -0.2, 1e-3, -2e-3]))
    c = t.get_seq_cfg(1)
    assert [c[k] for k in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2")] == [150.5, 151.5, 88.0, 96.0, 0.1, -0.2, 1e-3, -2e-3]
    assert t.get_seq_camera(1).as_dict() == {"model": 0, "proj": [150.5, 151.5, 88.0, 96.0], "dist": [0.1, -0.2, 1e-3, -2e-3], "xi": 0.0}
    t.close()


def test_untouched_handle_does_what_it_did(gf):
    """a handle that sets a PINHOLE through the wide setter: the bits, the counters and the stages of the profile of an untouched one; with a PINHOLE_FULL and a
    SCARAMUZZA sequence the launch sits inside the detection stage and no counter moves"""
    frames, depth = _frames()
    hs = [gf.FeatureTracker(gf.default_cfg(width=W, height=H, batch=2, **HANDLE)) for _ in range(3)]
    hs[1].set_seq_camera(1, hs[1].get_seq_camera(1, gf.CameraModelEx))
    full, sca, _, _ = _cameras(gf)
    hs[2].set_seq_camera(0, full); hs[2].set_seq_camera(1, sca)
    for h in hs:
        h.set_profiling(True)
    for k in range(4):
        r = [h.trackImageSome([0, 1], [DT * k] * 2, [frames[0][k], frames[1][k]], [depth] * 2) for h in hs]
        for b in range(2):
            assert np.array_equal(r[0][b][0], r[1][b][0]) and np.array_equal(r[0][b][1].view(np.uint64), r[1][b][1].view(np.uint64))
            assert np.array_equal(r[0][b][0], r[2][b][0]) and np.array_equal(r[0][b][1][:, [2, 3, 4, 7]].view(np.uint64), r[2][b][1][:, [2, 3, 4, 7]].view(np.uint64))
    c = [_counters(h) for h in hs]
    assert c[0] == c[1] == c[2] and c[0]["frames"] == 4
    s = [h.stats() for h in hs]
    assert all(x["ms_detect"] > 0 and x["ms_convert"] == 0 and x["ms_equalize"] == 0 for x in s)
    for h in hs:
        h.close()


if __name__ == "__main__" and "--host-lift-child" in sys.argv:
    import gfamd
    counters = _mixed_against_pinholes(gfamd, os.environ["GF_CAMERA_LIFT_HOST"])
    print("lift switched: ok (%d sequence frames)" % counters["sequence_frames"])
