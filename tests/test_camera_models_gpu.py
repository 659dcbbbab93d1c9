"""Camera models on the device: camera_lift_kernel through gf_camera_lift_batch / _device against the 60-digit fixture (tests/golden/camera_models.json.gz), and a
tracker handle whose sequences have a pinhole, a MEI and a Kannala-Brandt camera against pinhole handles on the same frames.

Bars (the fixture's eps_d is four times the error of the reference's own route in double precision): a ray component within eps_d max(1, |value|) of the 60-digit
value, a float pair within half a float ulp of it plus eps_d max(1, |value|).  In the tracker tests the 60-digit values come from the generator's functions
(tests/golden/make_camera_golden.py) on the pixels the tracker reports, and the velocities are recomputed from the reported pairs as ptsVelocity computes them
(feature_tracker.cpp:810-847: a float difference over a double dt, rounded to float).  Run with -m gpu."""
import ctypes as C
import gzip
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "ground-fusion_amd")):      # also where the module runs as the child process of test 5
    if _p not in sys.path:
        sys.path.insert(0, _p)
import synth  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "camera_models.json.gz")
DT = 0.0666
W, H, K = 320, 240, 5
HANDLE = dict(max_cnt=40, min_dist=20, flow_back=1, depth_cam=1)
MEI = ("MEI", [305.5, 306.25, 160.5, 120.25], [-0.02, 0.003, 2e-4, -1e-4], 1.3)
KB = ("KANNALA_BRANDT", [142.5, 143.25, 160.5, 120.25], [-0.9, 0.35, -0.05, 0.0025], 0.0)      # the fixture's `wiggle` polynomial: one and three roots inside the image
_G = {}


def _gen():
    """the generator's mpmath transcriptions, without its global precision"""
    if "g" not in _G:
        import mpmath
        import make_camera_golden as g
        mpmath.mp.dps = 15
        _G["g"], _G["mp"] = g, mpmath
    return _G["g"], _G["mp"]


def _fixture():
    if "doc" not in _G:
        _G["doc"] = json.loads(gzip.open(GOLDEN).read())
    return _G["doc"]


def _half_ulp32(v):
    a = np.maximum(np.abs(np.asarray(v, np.float64)), np.finfo(np.float32).tiny)
    return np.ldexp(0.5, np.floor(np.log2(a)).astype(int) - 23)


def _check(un, rays, exp, eps_d, what):
    """exp: rows of (ray hi [3], ray lo [3], pair hi [2], pair lo [2], pair_ok); rays may be None"""
    rhi, rlo, phi, plo, ok = exp
    if rays is not None:
        e = np.abs((rays - rhi) - rlo) / np.maximum(1.0, np.abs(rhi))
        assert e.max() <= eps_d, "%s: a ray component is off by %.3g of its scale (bar %.3g)" % (what, e.max(), eps_d)
    e = np.abs((un.astype(np.float64) - phi) - plo)[ok]
    bar = (_half_ulp32(phi) + eps_d * np.maximum(1.0, np.abs(phi)))[ok]
    assert (e <= bar).all(), "%s: a float pair is off by %.3g of its bar" % (what, (e / bar).max())


def _case_points(c):
    """the float pixels of a fixture case with what is expected of them"""
    pts = [p for p in c["points"] if not p["double_only"]]
    zero = [[0.0, 0.0], [0.0, 0.0]]
    uv = np.array([p["uv"] for p in pts], np.float32)
    ray = np.array([p["ray"] for p in pts])
    un = np.array([p.get("un", zero) for p in pts])
    return uv, (ray[:, :, 0], ray[:, :, 1], un[:, :, 0], un[:, :, 1], np.array([p["pair_ok"] for p in pts], bool))


def _pinhole_expected(proj, dist, uv):
    g, mp = _gen()
    with mp.workdps(60):
        rows = [g.mei_lift(proj, dist, 0.0, float(u), float(v)) for u, v in uv]      # xi = 0: (mx_u, my_u, 1), PinholeCamera.cc:450-510 has the same lines
        ray = np.array([[g.hilo(t) for t in P] for P in rows])
        un = np.array([[g.hilo(P[0] / P[2]), g.hilo(P[1] / P[2])] for P in rows])
    return ray[:, :, 0], ray[:, :, 1], un[:, :, 0], un[:, :, 1], np.ones(len(uv), bool)


def _batch(gf):
    """sequences of 150, 0, 150, 1, 63, 64, 65, ... points; neighbours always differ in their model; an empty sequence between two full ones"""
    if "batch" in _G:
        return _G["batch"]
    doc = _fixture()
    by = {c["name"]: c for c in doc["cases"]}
    pin = (gf.CameraModel.make("PINHOLE", [603.95556640625, 603.1257934570312, 324.0858154296875, 232.72303771972656], [0.148, -0.468, 1.6e-3, -8.9e-3]), None)
    order = ["kb_wiggle", "mei_xi1", "PINHOLE", "kb_neglead", "mei_xi199_dist", "kb_mono9", "PINHOLE", "mei_xi07_nodist", "kb_k2k3k4", "mei_xi0_dist", "kb_k2k3", "PINHOLE",
             "kb_k2", "mei_xi1", "kb_zero"]
    sizes = [150, 0, 150, 1, 63, 64, 65, 150, 64, 65, 63, 1, 150, 0, 64]
    cams, pts, exp = [], [], []
    rng = np.random.default_rng(5)
    for name, n in zip(order, sizes):
        if name == "PINHOLE":
            cam = pin[0]
            uv = np.stack([rng.uniform(0, 639, n), rng.uniform(0, 479, n)], 1).astype(np.float32)
            e = _pinhole_expected(list(cam.proj), list(cam.dist), uv)
        else:
            c = by[name]
            cam = gf.CameraModel.make(c["model"], c["proj"], c["dist"], c["xi"])
            uv0, e0 = _case_points(c)
            idx = np.arange(n) % len(uv0)
            uv, e = uv0[idx], tuple(a[idx] for a in e0)
        cams.append(cam); pts.append(uv); exp.append(e)
    assert all(a.model != b.model for a, b in zip(cams, cams[1:]))
    _G["batch"] = (cams, pts, exp, doc["eps_d"])
    return _G["batch"]


# ---- 1
def test_lift_batch_meets_the_fixture(gf):
    cams, pts, exp, eps_d = _batch(gf)
    un, rays = gf.camera_lift(cams, pts)
    for b in range(len(cams)):
        assert un[b].shape == (len(pts[b]), 2) and rays[b].shape == (len(pts[b]), 3)
        if len(pts[b]):
            _check(un[b], rays[b], exp[b], eps_d, "sequence %d (model %d, %d points)" % (b, cams[b].model, len(pts[b])))
    un2, none = gf.camera_lift(cams, pts, rays=False)      # the kernel writes no rays: the pairs keep their bits
    assert none is None and all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(un, un2))


def test_lift_batch_on_device_arrays(gf):
    import torch
    cams, pts, exp, eps_d = _batch(gf)
    flat = np.concatenate(pts)
    n = len(flat)
    d_uv = torch.from_numpy(flat).cuda()
    d_un = torch.full((n + 8, 2), -7.0, dtype=torch.float32, device="cuda")
    d_rays = torch.full((n + 8, 3), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    gf.camera_lift_device(cams, [len(p) for p in pts], d_uv.data_ptr(), d_rays.data_ptr(), d_un.data_ptr(), stream=s.cuda_stream)
    un, rays = d_un.cpu().numpy(), d_rays.cpu().numpy()
    assert (un[n:] == -7.0).all() and (rays[n:] == -7.0).all()      # nothing behind the last point
    host_un, host_rays = gf.camera_lift(cams, pts)
    assert np.array_equal(un[:n].view(np.uint32), np.concatenate(host_un).view(np.uint32)) and np.array_equal(rays[:n].view(np.uint64), np.concatenate(host_rays).view(np.uint64))
    at = 0
    for b in range(len(cams)):
        if len(pts[b]):
            _check(un[at:at + len(pts[b])], rays[at:at + len(pts[b])], exp[b], eps_d, "sequence %d" % b)
        at += len(pts[b])
    d_un.fill_(-7.0)
    torch.cuda.synchronize()
    gf.camera_lift_device(cams, [len(p) for p in pts], d_uv.data_ptr(), None, d_un.data_ptr())      # no rays, the null stream
    assert np.array_equal(d_un.cpu().numpy().view(np.uint32), un.view(np.uint32))


# ---- 2
def test_same_bits_twice_alone_and_behind_others(gf):
    cams, pts, _, _ = _batch(gf)
    a = gf.camera_lift(cams, pts)
    b = gf.camera_lift(cams, pts)
    for x, y in zip(a[0] + a[1], b[0] + b[1]):
        assert x.tobytes() == y.tobytes()
    for q in (0, 3, 4, 6, 12):
        un, rays = gf.camera_lift([cams[q]], [pts[q]])
        assert un[0].tobytes() == a[0][q].tobytes() and rays[0].tobytes() == a[1][q].tobytes(), "sequence %d alone" % q


# ---- 3
def test_non_finite_and_huge_coordinates(gf):
    """fixed bounds on every loop: the call returns, and the finite lanes of the same wavefront keep their bits"""
    cams, pts, _, _ = _batch(gf)
    sel = [0, 1, 2, 4, 5, 7]      # all three models; sequences of 150, 0, 150, 63, 64, 150 points
    clean = gf.camera_lift([cams[q] for q in sel], [pts[q] for q in sel])
    bad = [np.array(pts[q], copy=True) for q in sel]
    poison = [(np.nan, 10.0), (np.inf, np.inf), (-np.inf, 5.0), (1e30, -1e30), (3.0, np.nan), (1e30, 1e30), (-1e30, 0.0), (np.float32(3e38), np.float32(3e38))]
    lanes = []
    for p in bad:
        at = [i for i in (0, 5, 17, 31, 32, 62, 63, 64, 100, 149) if i < len(p)]
        for j, i in enumerate(at):
            p[i] = poison[j % len(poison)]
        lanes.append(at)
    un, rays = gf.camera_lift([cams[q] for q in sel], bad)
    for k in range(len(sel)):
        keep = np.ones(len(bad[k]), bool)
        keep[lanes[k]] = False
        assert np.array_equal(un[k][keep].view(np.uint32), clean[0][k][keep].view(np.uint32)) and np.array_equal(rays[k][keep].view(np.uint64), clean[1][k][keep].view(np.uint64))


# ---- 4: the tracker
def _frames():
    if "frames" not in _G:
        _G["frames"] = ([synth.tracker_sequence(s, K, W, H) for s in (2100, 2101, 2102)], np.full((H, W), 1500, np.uint16))
    return _G["frames"]


def _cameras(gf):
    return [None, gf.CameraModel.make(*MEI), gf.CameraModel.make(*KB)]


def _expected_pairs(model, uv):
    """the 60-digit pair (hi, lo) of every float pixel of uv, and whether the pair is compared"""
    g, mp = _gen()
    name, proj, dist, xi = model
    with mp.workdps(60):
        rows = [g.mei_lift(proj, dist, xi, float(u), float(v)) if name == "MEI" else g.kb_lift(proj, dist, float(u), float(v))[0] for u, v in uv]
        un = np.array([[g.hilo(P[0] / P[2]), g.hilo(P[1] / P[2])] for P in rows])
        ok = np.array([bool(abs(P[2]) / mp.sqrt(P[0] ** 2 + P[1] ** 2 + P[2] ** 2) >= 0.05) for P in rows])
    return un[:, :, 0], un[:, :, 1], ok


def _velocities(ids, un, prev, dt):
    """ptsVelocity (feature_tracker.cpp:810-847) on reported float pairs: prev = {id: pair} of the frame before, or None on the first frame"""
    v = np.zeros((len(ids), 2), np.float32)
    for i, fid in enumerate(ids):
        if prev is not None and int(fid) in prev:
            d = un[i] - prev[int(fid)]                                   # float - float
            v[i] = (d.astype(np.float64) / np.float64(dt)).astype(np.float32)
    return v


def _mixed_against_pinholes(gf, eps_d, check_60_digits=True):
    frames, depth = _frames()
    cams = _cameras(gf)
    mixed = gf.FeatureTracker(gf.default_cfg(width=W, height=H, batch=3, **HANDLE))
    for b in (1, 2):
        mixed.set_seq_camera(b, cams[b])
        assert mixed.get_seq_camera(b).as_dict() == cams[b].as_dict()
    own = mixed.get_seq_camera(0).as_dict()
    c = mixed.get_seq_cfg(0)
    assert own == {"model": 0, "proj": [c["fx"], c["fy"], c["cx"], c["cy"]], "dist": [c["k1"], c["k2"], c["p1"], c["p2"]], "xi": 0.0}      # ahead of any setter
    plain = [gf.FeatureTracker(gf.default_cfg(width=W, height=H, batch=1, **HANDLE)) for _ in range(3)]
    prev = [None] * 3
    carried = 0
    for k in range(K):
        L = [(k + i) % 3 for i in range(3)]      # the list in another order on every call
        ts = [DT * k + 0.001 * b for b in L]
        res = mixed.trackImageSome(L, ts, [frames[b][k] for b in L], [depth] * 3)
        for i, b in enumerate(L):
            ids, obs = res[i]
            pid, pobs = plain[b].trackImage(ts[i], frames[b][k], depth)
            what = "frame %d, sequence %d" % (k, b)
            assert np.array_equal(ids, pid), what + ": ids differ from the pinhole handle's"
            assert np.array_equal(obs[:, [2, 3, 4, 7]].view(np.uint64), pobs[:, [2, 3, 4, 7]].view(np.uint64)), what + ": pixel coordinates or depths differ"
            assert all(np.array_equal(x, y) for x, y in zip(mixed.state(b), plain[b].state())), what + ": ids / track counts / points of the state differ"
            if b == 0:
                assert np.array_equal(obs.view(np.uint64), pobs.view(np.uint64)), what + ": the pinhole sequence's output differs"
                continue
            assert (obs[:, 0:2] == obs[:, 0:2].astype(np.float32)).all() and (obs[:, 5:7] == obs[:, 5:7].astype(np.float32)).all()
            un = obs[:, 0:2].astype(np.float32)
            if check_60_digits:
                hi, lo, ok = _expected_pairs(MEI if b == 1 else KB, obs[:, 3:5])
                e = np.abs((un.astype(np.float64) - hi) - lo)[ok]
                bar = (_half_ulp32(hi) + eps_d * np.maximum(1.0, np.abs(hi)))[ok]
                assert ok.sum() >= 0.95 * len(ok) and (e <= bar).all(), what + ": a lifted pair is off by %.3g of its bar" % (e / bar).max()
            else:      # against the building block: the same kernel, the same bits
                blk = gf.camera_lift([cams[b]], [obs[:, 3:5]], rays=False)[0][0]
                assert np.array_equal(un.view(np.uint32), blk.view(np.uint32)), what + ": the tracker's pairs are not the building block's"
            dt = ts[i] - (DT * (k - 1) + 0.001 * b)
            want = _velocities(ids, un, prev[b], dt)
            assert np.array_equal(obs[:, 5:7].astype(np.float32).view(np.uint32), want.view(np.uint32)), what + ": velocities are not ptsVelocity of the lifted pairs"
            carried += 0 if prev[b] is None else sum(1 for f in ids if int(f) in prev[b])
            prev[b] = {int(f): un[j] for j, f in enumerate(ids)}
    assert carried > 3 * HANDLE["max_cnt"], "too few features were carried from frame to frame for the row index to matter"
    stats = mixed.stats()
    mixed.close()
    for p in plain:
        p.close()
    return stats


def test_tracker_with_three_models(gf):
    _mixed_against_pinholes(gf, _fixture()["eps_d"])


def test_tracker_pairs_are_the_building_blocks(gf):
    _mixed_against_pinholes(gf, _fixture()["eps_d"], check_60_digits=False)


# ---- 5
@pytest.mark.parametrize("host", ["1", "0"])
def test_tracker_with_the_lift_switched(host):
    """GF_CAMERA_LIFT_HOST is read when the tracker is created: a fresh child process runs the same comparison with the lift on the host (1) and, said
    explicitly, on the device (0)"""
    env = dict(os.environ, GF_CAMERA_LIFT_HOST=host)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--host-lift-child"], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0 and "host lift: ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


# ---- 6
def test_set_prediction_goes_through_the_model(gf):
    """predictions for the Kannala-Brandt sequence are rays lifted from float pixel targets; a pinhole handle gets points that project to the same float pixels:
    the next frame is the same, bit for bit, in everything that does not depend on the model"""
    frames, depth = _frames()
    kb = gf.CameraModel.make(*KB)
    a = gf.FeatureTracker(gf.default_cfg(width=W, height=H, batch=1, **HANDLE))
    a.set_seq_camera(0, kb)
    b = gf.FeatureTracker(gf.default_cfg(width=W, height=H, batch=1, **HANDLE))
    par = b.get_seq_cfg(0)
    rng = np.random.default_rng(3)
    for k in range(4):
        ia, oa = a.trackImage(DT * k, frames[2][k], depth)
        ib, ob = b.trackImage(DT * k, frames[2][k], depth)
        assert np.array_equal(ia, ib) and np.array_equal(oa[:, [2, 3, 4, 7]].view(np.uint64), ob[:, [2, 3, 4, 7]].view(np.uint64)), "frame %d" % k
        assert all(np.array_equal(x, y) for x, y in zip(a.state(), b.state()))
        ids, _, pts = a.state()
        sel = rng.random(len(ids)) < 0.7
        target = (pts[sel] + rng.normal(0, 1.0, (int(sel.sum()), 2))).astype(np.float32)
        rays = gf.camera_lift([kb], [target])[1][0]
        back = gf.camera_project([kb], [rays])[0]
        assert np.array_equal(back.astype(np.float32), target), "a lifted target does not project back onto its float pixel"
        t64 = target.astype(np.float64)
        xyz = np.stack([(t64[:, 0] - par["cx"]) / par["fx"] * 2.0, (t64[:, 1] - par["cy"]) / par["fy"] * 2.0, np.full(len(t64), 2.0)], 1)
        pin = gf.camera_project([b.get_seq_camera(0)], [xyz])[0]
        assert np.array_equal(pin.astype(np.float32), target)
        a.setPrediction(ids[sel], rays * 3.0, seq=0)      # any point on the ray
        b.setPrediction(ids[sel], xyz, seq=0)
    assert a.stats()["lk_launches"] == b.stats()["lk_launches"] and len(ia) > 20
    a.close(); b.close()


# ---- 7
def test_setter_rules(gf):
    import torch
    frames, depth = _frames()
    lib = gf.lib()
    kb, mei = gf.CameraModel.make(*KB), gf.CameraModel.make(*MEI)
    t = gf.FeatureTracker(gf.default_cfg(width=W, height=H, batch=2, **HANDLE))
    assert lib.gf_tracker_set_seq_camera(None, 0, C.byref(kb)) == -1 and lib.gf_tracker_get_seq_camera(None, 0, C.byref(kb)) == -1
    for seq in (-1, 2):
        with pytest.raises(gf.GfError, match="gf status -1.*sequence %d of a handle of 2" % seq):
            t.set_seq_camera(seq, kb)
    for field, bad in (("xi", gf.CameraModel.make("MEI", MEI[1], MEI[2], -0.5)), ("gamma1", gf.CameraModel.make("MEI", [0.0, 300, 160, 120])),
                       ("k3", gf.CameraModel.make("KANNALA_BRANDT", KB[1], [-0.1, 0.0, 0.0, 1e-3])), ("mv", gf.CameraModel.make("KANNALA_BRANDT", [140.0, float("nan"), 160, 120])),
                       ("model", gf.CameraModel.make(5, KB[1]))):
        with pytest.raises(gf.GfError, match="gf status -1.*%s" % field):
            t.set_seq_camera(1, bad)
    t.set_seq_camera(1, kb)
    # a pinhole through this setter is the eight fields of the sequence's parameters
    t.set_seq_camera(0, gf.CameraModel.make("PINHOLE", [600.5, 601.5, 161.0, 119.0], [0.1, -0.2, 1e-3, -2e-3]))
    c = t.get_seq_cfg(0)
    assert [c[k] for k in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2")] == [600.5, 601.5, 161.0, 119.0, 0.1, -0.2, 1e-3, -2e-3] and c["max_cnt"] == HANDLE["max_cnt"]
    before = t.get_seq_cfg(1)
    t.trackImageSome([1], [0.0], [frames[0][0]], [depth])
    with pytest.raises(gf.GfError, match="gf status -1.*sequence 1 has taken a frame"):
        t.set_seq_camera(1, mei)
    assert t.get_seq_camera(1).as_dict() == kb.as_dict() and t.get_seq_cfg(1) == before      # the parameters' camera fields stay stored
    t.reset_seq(1)
    assert t.get_seq_camera(1).as_dict() == kb.as_dict()      # a setting: kept by the reset, and settable again
    t.set_seq_camera(1, mei)
    g = torch.from_numpy(np.ascontiguousarray(frames[0][0])).pin_memory()
    d = torch.from_numpy(depth.view(np.int16)).pin_memory()
    t.prefetchHost([g.data_ptr()], [d.data_ptr()], seqs=[1])
    with pytest.raises(gf.GfError, match="gf status -1.*sequence 1 is listed by a staged frame"):
        t.set_seq_camera(1, kb)
    t.trackPrefetched([0.0])
    assert t.get_seq_camera(1).as_dict() == mei.as_dict()
    # back to a pinhole: the stored fields are in force again
    t.reset_seq(1)
    t.set_seq_camera(1, gf.CameraModel.make("PINHOLE", [before[k] for k in ("fx", "fy", "cx", "cy")], [before[k] for k in ("k1", "k2", "p1", "p2")]))
    p = gf.FeatureTracker(gf.default_cfg(width=W, height=H, batch=1, **HANDLE))
    for k in range(2):
        x = t.trackImageSome([1], [DT * k], [frames[1][k]], [depth])[0]
        y = p.trackImage(DT * k, frames[1][k], depth)
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[1].view(np.uint64), y[1].view(np.uint64))
    t.close(); p.close()


# ---- 8
def test_untouched_handle_does_what_it_did(gf):
    """a handle that sets no camera, and one that sets a pinhole through the new setter: the bits, the counters and the stages of the profile of an untouched one"""
    frames, depth = _frames()
    hs = [gf.FeatureTracker(gf.default_cfg(width=W, height=H, batch=2, **HANDLE)) for _ in range(2)]
    c = hs[1].get_seq_camera(1)
    hs[1].set_seq_camera(1, c)
    for h in hs:
        h.set_profiling(True)
    for k in range(K):
        r = [h.trackImageSome([0, 1], [DT * k] * 2, [frames[0][k], frames[1][k]], [depth] * 2) for h in hs]
        for b in range(2):
            assert np.array_equal(r[0][b][0], r[1][b][0]) and np.array_equal(r[0][b][1].view(np.uint64), r[1][b][1].view(np.uint64))
    s = [h.stats() for h in hs]
    counters = [k for k in s[0] if not k.startswith("ms_")]
    assert {k: s[0][k] for k in counters} == {k: s[1][k] for k in counters}
    assert s[0]["frames"] == K and s[0]["ms_detect"] > 0 and s[0]["ms_convert"] == 0 and s[0]["ms_equalize"] == 0
    # with a model set, the launch sits inside the detection stage of the profile, and nothing else of the counters moves
    m = gf.FeatureTracker(gf.default_cfg(width=W, height=H, batch=2, **HANDLE))
    m.set_seq_camera(1, gf.CameraModel.make(*KB))
    m.set_profiling(True)
    for k in range(K):
        m.trackImageSome([0, 1], [DT * k] * 2, [frames[0][k], frames[1][k]], [depth] * 2)
    sm = m.stats()
    assert {k: sm[k] for k in counters} == {k: s[0][k] for k in counters} and sm["ms_detect"] > 0
    for h in hs + [m]:
        h.close()


# ---- 9
def test_estimator_camera_and_replay(gf, tmp_path):
    """gf_estimator_set_camera on an estimator's own tracker, and bin/gf_replay from a config whose cam0_calib is a MEI file: it runs to a vio.txt, the one of
    the pinhole file that describes the same optics"""
    import synth_stream as SS
    st = SS.Stream(1, t_still=1.5, t_move=1.0, v_max=0.4, yaw0=0.0, yaw_turn=-0.6, split_x=1.8, turn_delay=0.8)
    d = str(tmp_path)
    n = st.export(d)
    cfg_path = os.path.join(d, "config.yaml")
    cfg = gf.estimator_cfg_from_yaml(cfg_path)
    calib = [l.split(":", 1)[1].strip().strip('"') for l in open(cfg_path) if l.startswith("cam0_calib")][0]
    t = cfg.tracker
    exe = os.path.join(ROOT, "bin", "gf_replay")
    first = subprocess.run([exe, cfg_path, d, os.path.join(d, "vio_pinhole.txt")], capture_output=True, text=True, timeout=600)
    assert first.returncode == 0, first.stderr
    # the same optics written as a MEI camera with xi = 0: the trajectory of the pinhole run, through the other model's code and the device lift
    open(os.path.join(d, calib), "w").write("%%YAML:1.0\n---\nmodel_type: MEI\ncamera_name: camera\nimage_width: %d\nimage_height: %d\nmirror_parameters:\n   xi: 0.0\n"
                                           "distortion_parameters:\n   k1: %r\n   k2: %r\n   p1: %r\n   p2: %r\nprojection_parameters:\n   gamma1: %r\n   gamma2: %r\n   u0: %r\n   v0: %r\n"
                                           % (t.width, t.height, t.k1, t.k2, t.p1, t.p2, t.fx, t.fy, t.cx, t.cy))
    with pytest.raises(gf.GfError, match="only PINHOLE is built"):
        gf.estimator_cfg_from_yaml(cfg_path)
    cfg2, cam = gf.estimator_cfg_from_yaml_camera(cfg_path)
    assert cam.model == gf.CAMERA_MEI and cam.xi == 0.0 and list(cam.proj) == [t.fx, t.fy, t.cx, t.cy]
    est = gf.SlidingWindowEstimator(cfg2)
    est.set_camera(cam)
    gray, depth = st.image(0)
    est.inputImage(float(st.cam_t[0]), gray, depth)
    with pytest.raises(gf.GfError, match="has taken a frame"):
        est.set_camera(cam)
    est.close()
    out = subprocess.run([exe, cfg_path, d, os.path.join(d, "vio.txt")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    assert "%d RGB-D pairs (0 / 0 unpaired" % n in out.stdout
    got = np.loadtxt(os.path.join(d, "vio.txt"))
    assert got.ndim == 2 and got.shape[1] == 8 and len(got) > 5 and np.isfinite(got).all()
    # xi = 0 without distortion: the ray is (mx, my, 1 - 0) in the same IEEE operations as the pinhole's, so the whole replay is the pinhole's
    assert open(os.path.join(d, "vio.txt"), "rb").read() == open(os.path.join(d, "vio_pinhole.txt"), "rb").read()


if __name__ == "__main__" and "--host-lift-child" in sys.argv:
    import gfamd
    # on the host the pairs are held to the 60-digit formulas; on the device they are the building block's, which test 1 holds to them
    stats = _mixed_against_pinholes(gfamd, _fixture()["eps_d"], check_60_digits=os.environ.get("GF_CAMERA_LIFT_HOST") == "1")
    print("host lift: ok (%d frames)" % stats["frames"])
