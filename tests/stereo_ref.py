"""TEST INFRASTRUCTURE: the stereo branch of FeatureTracker::trackImage (feature_tracker.cpp:259-303, kept there commented out) restated in numpy around the oracle:
oracle_py.Tracker is the left branch and its state(), oracle_py.lk on (left, right) and (right, left) the two passes of the stage, and the right-hand lists, maps,
velocities and the packing are written out here as DESIGN.md section 4, "Stereo", defines them.  Also the scenes the stereo tests share and their census."""
import numpy as np

import roi_ref as RR

K = 6
SHIFTS = (3, 7, 12)          # px each third of the rows is moved to the left in the right frame
PATCH_W, PATCH_H = 20, 16    # a flat patch of 128 over the centre of the right frame only
CASES = [RR.SIZES[0], RR.SIZES[2]]   # (w, h, max_cnt, min_dist): 132 x 97 and 64 x 61
MIXED = RR.SIZES[1]                  # 188 x 122, the handle of the mixed-size case
# a right camera the tests share: the distorted pinhole of test_track_host's distort=1 case (config/realsense/idc_cam.yaml)
RIGHT_PROJ = (6.2097277909374247e+02, 6.2212293397677581e+02, 3.1175896455154810e+02, 2.4718077836114819e+02)
RIGHT_DIST = (1.4865749308203452e-01, -4.6815685578576460e-01, 1.6205585303208318e-03, -8.9101576735577930e-03)


def stamp(k):
    """the time of a sequence's frame k: no two frame intervals are equal, so a velocity taken over the wrong dt shows"""
    return 0.0666 * k + 0.001 * k * k


def right_frame(left, k):
    """the right frame of frame k: three bands of rows shifted left by 3, 7, 12 px, over a frame of seeded bytes (which the freed columns keep), a flat patch over the centre"""
    h, w = left.shape
    R = np.random.default_rng(700 + k).integers(0, 256, (h, w), dtype=np.uint8)   # one frame of seeded bytes: what the shifts do not cover stays
    for i, d in enumerate(SHIFTS):
        a, b = i * h // 3, (i + 1) * h // 3
        R[a:b, :w - d] = left[a:b, d:]
    x0, y0 = w // 2 - PATCH_W // 2, h // 2 - PATCH_H // 2
    R[y0:y0 + PATCH_H, x0:x0 + PATCH_W] = 128
    return np.ascontiguousarray(R)


_SCENES = {}


def scene(w, h):
    """(left frames, right frames) of a size, six each; built once per process and never written to"""
    if (w, h) not in _SCENES:
        left = [np.ascontiguousarray(f, np.uint8) for f in RR.frames(w, h, n=K)]
        right = [right_frame(f, k) for k, f in enumerate(left)]
        for f in left + right:
            f.setflags(write=False)
        _SCENES[(w, h)] = (left, right)
    return _SCENES[(w, h)]


def in_border(pts, w, h):
    """inBorder (feature_tracker.cpp:14-20): cvRound of the float coordinates, BORDER_SIZE 1"""
    x, y = np.rint(pts[:, 0]).astype(np.int64), np.rint(pts[:, 1]).astype(np.int64)
    return (1 <= x) & (x < w - 1) & (1 <= y) & (y < h - 1)


def match(oracle, left, right, pts, flow_back):
    """steps 2 and 3 of the stage on all of pts -> (right points, status, forward status, parts): both passes with maxLevel 3 and no initial flow; parts holds the
    four terms of the conjunction (forward, reverse, inBorder, distance) for the census"""
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
    h, w = left.shape
    if len(pts) == 0:
        z = np.zeros(0, np.uint8)
        return np.zeros((0, 2), np.float32), z, z, None
    rp, fwd, _ = oracle.lk(left, right, pts, None, 3)
    if not flow_back:
        return rp, fwd.copy(), fwd, None
    back, rev, _ = oracle.lk(right, left, rp, None, 3)
    d = pts - back                                                         # float differences, the norm in double (distance(), feature_tracker.cpp:22-28)
    near = np.sqrt(d[:, 0].astype(np.float64) ** 2 + d[:, 1].astype(np.float64) ** 2) <= 0.5
    inb = in_border(rp, w, h)
    st = ((fwd > 0) & (rev > 0) & inb & near).astype(np.uint8)
    return rp, st, fwd, dict(fwd=fwd > 0, rev=rev > 0, inb=inb, near=near)


def pinhole_lift(proj, dist, pts):
    """PinholeCamera::liftProjective as gf_camera_models.hpp's undistort writes it, operation for operation in float64, then the float pair of undistortedPts"""
    fx, fy, cx, cy = [np.float64(v) for v in proj]
    k1, k2, p1, p2 = [np.float64(v) for v in dist[:4]]
    u, v = pts[:, 0].astype(np.float64), pts[:, 1].astype(np.float64)
    i11, i13, i22, i23 = 1.0 / fx, -cx / fx, 1.0 / fy, -cy / fy
    mx_d, my_d = i11 * u + i13, i22 * v + i23

    def distortion(x, y):
        mx2, my2, mxy = x * x, y * y, x * y
        rho2 = mx2 + my2
        rad = k1 * rho2 + k2 * rho2 * rho2
        return x * rad + 2.0 * p1 * mxy + p2 * (rho2 + 2.0 * mx2), y * rad + 2.0 * p2 * mxy + p1 * (rho2 + 2.0 * my2)
    if k1 == 0 and k2 == 0 and p1 == 0 and p2 == 0:
        X, Y = mx_d, my_d
    else:
        dx, dy = distortion(mx_d, my_d)
        X, Y = mx_d - dx, my_d - dy
        for _ in range(7):
            dx, dy = distortion(X, Y)
            X, Y = mx_d - dx, my_d - dy
    return np.stack([(X / 1.0).astype(np.float32), (Y / 1.0).astype(np.float32)], 1)


class Tracker:
    """one stereo sequence.  lift: [n, 2] float32 right points -> [n, 2] float32 pairs through the right camera.  track() returns (ids, camera ids, observations
    [n, 8] float64): the left observations as the oracle's Tracker gives them, then one per entry of ids_right."""

    def __init__(self, oracle, max_cnt, min_dist, flow_back, lift):
        self.oracle, self.cfg, self.flow_back, self.lift = oracle, (max_cnt, min_dist, flow_back), flow_back, lift
        self.reset()

    def reset(self):
        max_cnt, min_dist, flow_back = self.cfg
        self.o = self.oracle.Tracker(self.oracle.default_cfg(max_cnt=max_cnt, min_dist=min_dist, flow_back=flow_back, depth_cam=0))
        self.prev_time = 0.0
        self.ids_right = np.zeros(0, np.int32)
        self.cur_right_pts = np.zeros((0, 2), np.float32)
        self.prev_un_right_pts_map = {}
        self.census = dict(points=0, fwd_fail=0, rev_fail=0, border=0, distance_alone=0, kept=0)

    def remove_outliers(self, ids):
        self.o.remove_outliers(np.asarray(ids, np.int32))   # the left lists only, as in the reference

    def state(self):
        return self.o.state()

    def track(self, t, left, right):
        ids, obs = self.o.track(t, left, None)
        sids, _, cur_pts = self.o.state()     # after the roll-over prev_pts holds the frame's cur_pts, in the order of ids
        assert np.array_equal(ids, sids)
        cam = np.zeros(len(ids), np.int32)
        dt = np.float64(t) - np.float64(self.prev_time)
        self.prev_time = t
        if right is None:                     # `!_img1.empty()`: the stage is skipped, the right-hand state stays
            return ids, cam, obs
        self.ids_right, self.cur_right_pts = np.zeros(0, np.int32), np.zeros((0, 2), np.float32)
        cur_map, un, vel = {}, np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32)
        if len(cur_pts):
            rp, st, fwd, parts = match(self.oracle, left, right, cur_pts, self.flow_back)
            keep = st > 0
            c = self.census
            c["points"] += len(st); c["kept"] += int(keep.sum())
            if parts is not None:
                f, r, b, n = parts["fwd"], parts["rev"], parts["inb"], parts["near"]
                c["fwd_fail"] += int((~f).sum()); c["rev_fail"] += int((f & ~r).sum())
                c["border"] += int((f & r & ~b).sum()); c["distance_alone"] += int((f & r & b & ~n).sum())
            else:
                c["fwd_fail"] += int((fwd == 0).sum())
            self.ids_right, self.cur_right_pts = sids[keep].copy(), rp[keep].copy()
            un = np.ascontiguousarray(self.lift(self.cur_right_pts), np.float32).reshape(-1, 2)
            vel = np.zeros_like(un)
            if self.prev_un_right_pts_map:
                for i, f in enumerate(self.ids_right):
                    p = self.prev_un_right_pts_map.get(int(f))
                    if p is not None:
                        vel[i] = ((un[i] - p).astype(np.float64) / dt).astype(np.float32)
            cur_map = {int(f): un[i].copy() for i, f in enumerate(self.ids_right)}
        self.prev_un_right_pts_map = cur_map
        n = len(self.ids_right)
        robs = np.zeros((n, 8), np.float64)
        robs[:, 0:2] = un; robs[:, 2] = 1; robs[:, 3:5] = self.cur_right_pts; robs[:, 5:7] = vel; robs[:, 7] = -2.4
        return (np.concatenate([ids, self.ids_right]).astype(np.int32), np.concatenate([cam, np.ones(n, np.int32)]),
                np.concatenate([obs, robs]) if n else obs)
