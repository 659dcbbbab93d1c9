"""Windows that take every branch and input class of the visual, IMU and wheel factors (csrc/gf_ba_kernels.hpp: visual_eval, huber_corrector, vis_lane_cost, the IMU and
wheel evaluations, prior_block_dx; csrc/gf_dmath.hpp: so3_exp, so3_log, rightJacobianSO3, rightJacobianInvSO3; the sum_dt switch of MARGIN_OLD).  Plain numpy, no GPU.

Every window the back-end tests had comes from synth_window.make_window as it stands: 95-98 % of the visual factors are Huber outliers at the first linearisation, the
velocity and the time offset of a track's first observation are exactly zero, every pose is within 11 degrees of the identity with w > 0.995, the wheel factors sit on
their linearisation point, inverse depths lie in 0.097 .. 0.68, the biases are 0.005 / 0.0005 from theirs, positions within metres of the origin.  The cases here are
make_window windows of the small size plus edits; `census_of` restates the BRANCH DECISIONS of the factors in numpy (the values come from
tests/golden/make_ref_golden.py at 60 digits) and counts, per window, how many factors take each side of each switch and how far each factor is from it: the cases are
chosen so that double and 60-digit arithmetic decide alike (MARGIN).

  python tests/factor_hard_cases.py      writes profiles/factor_hard_census.json (the new cases and the older inputs side by side)

tests/test_factor_hard_cases_host.py holds the census to its conditions and to the committed file; tests/test_factor_hard_cases_gpu.py runs the cases on the device."""
import gzip
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (os.path.join(ROOT, "ground-fusion_amd"), os.path.join(ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

SMALL = dict(max_features=6, n_landmarks=9)          # the size of tests/golden/ref_window_wheel
MID = dict(max_features=8, n_landmarks=12)
MARG = dict(max_features=10, n_landmarks=15)         # the size of tests/golden/ref_marg_old_with_prior
MARGIN = 1e-9                                         # no factor nearer to a switch than this (relative to the switch; absolute for the sign switches)


# ---------------------------------------------------------------- quaternions as (w, x, y, z), numpy
def qmul(a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw])


def qinv(q):
    return np.array([q[0], -q[1], -q[2], -q[3]]) / (q @ q)


def qmat(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def qexp(v):
    th = np.linalg.norm(v)
    if th == 0:
        return np.array([1.0, 0, 0, 0])
    return np.concatenate([[np.cos(th / 2)], np.sin(th / 2) / th * np.asarray(v)])


def qlog(q):
    q = q / np.linalg.norm(q)
    n = np.linalg.norm(q[1:])
    return np.zeros(3) if n == 0 else 2 * np.arctan(n / q[0]) / n * q[1:]


def pose_q(w, i, key="para_Pose"):
    p = w[key][7 * i:7 * i + 7]
    return np.array([p[6], p[3], p[4], p[5]])


def set_pose_q(w, i, q, key="para_Pose"):
    w[key][7 * i + 3:7 * i + 7] = [q[1], q[2], q[3], q[0]]


# ---------------------------------------------------------------- a window's visual lists as tracks, and back
def tracks_of(w):
    """per feature: first frame, its observation there (point, velocity, time offset: one of each per feature, as the device stores them), inverse depth, the fixed flag, and
    the later observations (frame, point, velocity, time offset)"""
    out = []
    for f in range(int(w["n_feature"])):
        idx = np.nonzero(w["vis_feature"] == f)[0]
        k0 = idx[0]
        out.append({"start": int(w["vis_i"][k0]), "pts_i": w["vis_pts_i"][3 * k0:3 * k0 + 3].copy(), "vel_i": w["vis_vel_i"][2 * k0:2 * k0 + 2].copy(), "td_i": float(w["vis_td_i"][k0]),
                    "inv_dep": float(w["para_Feature"][f]), "fixed": int(w["feature_fixed"][f]),
                    "obs": [(int(w["vis_j"][k]), w["vis_pts_j"][3 * k:3 * k + 3].copy(), w["vis_vel_j"][2 * k:2 * k + 2].copy(), float(w["vis_td_j"][k])) for k in idx]})
    return out


def set_tracks(w, tracks):
    vf, vi, vj, pi_, pj_, vli, vlj, tdi, tdj = [], [], [], [], [], [], [], [], []
    for f, t in enumerate(tracks):
        for (j, pts_j, vel_j, td_j) in t["obs"]:
            vf.append(f); vi.append(t["start"]); vj.append(j); pi_.append(t["pts_i"]); pj_.append(pts_j); vli.append(t["vel_i"]); vlj.append(vel_j); tdi.append(t["td_i"]); tdj.append(td_j)
    w["vis_feature"], w["vis_i"], w["vis_j"] = vf, vi, vj
    w["vis_pts_i"], w["vis_pts_j"], w["vis_vel_i"], w["vis_vel_j"] = np.array(pi_), np.array(pj_), np.array(vli), np.array(vlj)
    w["vis_td_i"], w["vis_td_j"] = np.array(tdi), np.array(tdj)
    w["para_Feature"], w["feature_fixed"] = np.array([t["inv_dep"] for t in tracks]), np.array([t["fixed"] for t in tracks], np.uint8)
    return w.finalize()


def visual_geometry(w):
    """projectionTwoFrameOneCamFactor.cpp:61-77 in numpy: per factor the point in camera j, its projection and the whitened residual"""
    qic, tic = pose_q(w, 0, "para_Ex_Pose"), w["para_Ex_Pose"][0:3]
    ric, td, si = qmat(qic), float(w["para_Td"][0]), float(w["vis_sqrt_info"])
    out = []
    for k in range(int(w["n_visual"])):
        f, i, j = int(w["vis_feature"][k]), int(w["vis_i"][k]), int(w["vis_j"][k])
        vel_i, vel_j = np.append(w["vis_vel_i"][2 * k:2 * k + 2], 0), np.append(w["vis_vel_j"][2 * k:2 * k + 2], 0)
        pts_i = w["vis_pts_i"][3 * k:3 * k + 3] - (td - w["vis_td_i"][k]) * vel_i
        pts_j = w["vis_pts_j"][3 * k:3 * k + 3] - (td - w["vis_td_j"][k]) * vel_j
        Ri, Rj = qmat(pose_q(w, i)), qmat(pose_q(w, j))
        Xw = Ri @ (ric @ (pts_i / w["para_Feature"][f]) + tic) + w["para_Pose"][7 * i:7 * i + 3]
        Xj = ric.T @ (Rj.T @ (Xw - w["para_Pose"][7 * j:7 * j + 3]) - tic)
        proj = Xj[:2] / Xj[2]
        r = si * (proj - pts_j[:2])
        out.append({"Xj": Xj, "proj": proj, "r": r, "sq": float(r @ r)})
    return out


# ---------------------------------------------------------------- the edits
def turn(w, angle_deg=205.0, axis=(0.36, -0.48, 0.8), shift=(4000.0, -3000.0, 1500.0)):
    """every pose, every velocity and G turned by one rotation about a tilted axis, positions shifted: the window in another world frame"""
    q0 = qexp(np.radians(angle_deg) * np.asarray(axis) / np.linalg.norm(axis))
    R0 = qmat(q0)
    for i in range(int(w["W"]) + 1):
        w["para_Pose"][7 * i:7 * i + 3] = R0 @ w["para_Pose"][7 * i:7 * i + 3] + np.asarray(shift)
        set_pose_q(w, i, qmul(q0, pose_q(w, i)))
        w["para_SpeedBias"][9 * i:9 * i + 3] = R0 @ w["para_SpeedBias"][9 * i:9 * i + 3]
    w["G"] = R0 @ w["G"]
    return w


def spread_td(w, seed):
    """para_Td off zero and free, a time offset per feature (first observation) and per factor, a velocity of the first observation per feature"""
    rng = np.random.default_rng(seed * 811 + 3)
    w["para_Td"][0], w["fix_td"] = 0.012, 0
    tr = tracks_of(w)
    for t in tr:
        t["td_i"], t["vel_i"] = float(rng.uniform(-0.01, 0.02)), rng.uniform(0.05, 0.4, 2) * rng.choice([-1.0, 1.0], 2)
        t["obs"] = [(j, p, v, float(rng.uniform(-0.01, 0.02))) for (j, p, v, _) in t["obs"]]
    return set_tracks(w, tr)


def wheel_off(w, td_wheel):
    """every wheel pre-integration linearised off the defaults, the intrinsics and the time offset away from that point, all four free"""
    nw = int(w["n_wheel"])
    w["wh_lin"] = np.tile([1.02, 0.97, 1.01, 0.004], nw)
    w["para_Ix"][:] = [1.043, 0.951, 1.052]
    w["para_Td_wheel"][0] = td_wheel
    w["fix_ix"], w["fix_td_wheel"] = 0, 0
    return w


def wheel_rest(w):
    """pose j of two wheel factors from the factor's own delta_q (the intrinsics and td sit on the linearisation point: delta_q_time = delta_q), times a rotation of
    5e-12 rad (factor 2) and 1e-7 rad (factor 6): raw rotation residuals below 1e-10 and between 1e-10 and 1e-5"""
    qio = pose_q(w, 0, "para_Ex_Pose_wheel")
    for k, ang in ((2, 5e-12), (6, 1e-7)):
        dq = w["wh_delta_q"][4 * k:4 * k + 4]
        d = qexp(ang * np.array([0.6, -0.64, 0.48]))
        q = qmul(qmul(qmul(qmul(pose_q(w, k), qio), dq / np.linalg.norm(dq)), d), qinv(qio))
        set_pose_q(w, k + 1, q / np.linalg.norm(q))
    return w


def depth_extremes(w):
    """inverse depths 1e-3 (a far point), 5 (20 cm), -0.05 (behind the camera: the solver passes through such values), and one depth chosen so that the feature's last
    observation has it 3 .. 10 cm in front of camera j.  The feature that gets each value is the first one for which no factor of the window comes within 2 mm of z = 0 (at 1 m/s and 15 Hz a point 20 cm ahead is passed between the third and the fourth frame)."""
    tr = tracks_of(w)
    free = list(range(len(tr)))
    for val in (1e-3, 5.0, -0.05):
        for f in free:
            old = tr[f]["inv_dep"]
            tr[f]["inv_dep"] = val
            z = [g["Xj"][2] for g, k in zip(visual_geometry(set_tracks(w, tr)), w["vis_feature"]) if k == f]
            if min(abs(x) for x in z) > 2e-3:
                free.remove(f)
                break
            tr[f]["inv_dep"] = old
        else:
            raise AssertionError("no feature takes inverse depth %g" % val)
    for f in free:       # near: bisect on the depth of the feature until its last factor sees it at 6 cm
        old = tr[f]["inv_dep"]
        lo, hi = 0.05, 20.0
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            tr[f]["inv_dep"] = 1.0 / mid
            z = [g["Xj"][2] for g, k in zip(visual_geometry(set_tracks(w, tr)), w["vis_feature"]) if k == f]
            lo, hi = (mid, hi) if z[-1] < 0.06 else (lo, mid)
        if 0.03 < z[-1] < 0.1 and min(z) > 0.03:
            return set_tracks(w, tr)
        tr[f]["inv_dep"] = old
    raise AssertionError("no feature can be brought within 10 cm of a camera")


def track_shapes(w):
    """one feature seen in all W + 1 frames stays; one with at least 5 observations is cut to exactly 4; one whose track reaches frame W is re-anchored at frame W - 3 (its
    observation there becomes the first one, velocity and all, its inverse depth the one the old factor saw there) and goes to the end of the list (latest start)"""
    W = int(w["W"])
    tr = tracks_of(w)
    geo = visual_geometry(w)
    k0 = np.cumsum([0] + [len(t["obs"]) for t in tr])
    full = [f for f, t in enumerate(tr) if t["start"] == 0 and len(t["obs"]) == W]
    assert full, "no feature is seen in every frame"
    late = [f for f, t in enumerate(tr) if f != full[0] and t["obs"][-1][0] == W and t["start"] < W - 3]
    cut = [f for f, t in enumerate(tr) if f not in (full[0], late[0]) and len(t["obs"]) >= 4]
    t = tr[cut[0]]
    t["obs"] = t["obs"][:3]
    t = tr.pop(late[0])
    q = [o[0] for o in t["obs"]].index(W - 3)
    j, p, v, tdj = t["obs"][q]
    tr.append({"start": W - 3, "pts_i": p, "vel_i": v, "td_i": tdj, "inv_dep": 1.0 / float(geo[k0[late[0]] + q]["Xj"][2]), "fixed": t["fixed"], "obs": t["obs"][q + 1:]})
    return set_tracks(w, tr)


def far_bias(w):
    """Ba - lin_ba about 0.3 and Bg - lin_bg about 0.05 in every frame.  IMU interval 0 and wheel interval 5 are given sum_dt = 9.99, IMU interval 5 and wheel interval 0
    sum_dt = 10.01 (MARGIN_OLD reads the switch, for interval 0: it keeps the IMU factor and skips the wheel factor).  delta_p and delta_v of the two IMU intervals get the
    gravity and velocity terms of the longer time added, so that the residuals stay those of a window and not 490 m of free fall"""
    NP = int(w["W"]) + 1
    sb = w["para_SpeedBias"].reshape(NP, 9)
    sb[:, 3:6] += [0.3, -0.27, 0.24]
    sb[:, 6:9] += [0.05, -0.04, 0.045]
    for k, T in ((0, 9.99), (5, 10.01)):
        i = int(w["imu_i"][k])
        t = float(w["imu_sum_dt"][k])
        Rit = qmat(pose_q(w, i)).T
        w["imu_delta_p"][3 * k:3 * k + 3] += Rit @ (0.5 * w["G"] * (T * T - t * t) - sb[i, 0:3] * (T - t))
        w["imu_delta_v"][3 * k:3 * k + 3] += Rit @ (w["G"] * (T - t))
        w["imu_sum_dt"][k] = T
        # ... and the covariance grows as that of a longer integration does (white noise: velocity, rotation and biases with sqrt(T), position with T^1.5), so that the
        # factor is not 150 times a short interval's weight on a 150 times longer lever
        s = np.sqrt(T / t) * np.ones(15)
        s[0:3] = (T / t) ** 1.5
        w["imu_covariance"][225 * k:225 * k + 225] = (w["imu_covariance"][225 * k:225 * k + 225].reshape(15, 15) * np.outer(s, s)).reshape(-1)
    w["wh_sum_dt"][0], w["wh_sum_dt"][5] = 10.01, 9.99
    return w


def blend(seed, pre, s, kw):
    """the states of the unperturbed window plus s times the perturbation make_window adds (the measurements are those of either)"""
    import synth_window as SW
    P, U = SW.make_window(seed, pre, **kw).finalize(), SW.make_window(seed, pre, perturb=False, **kw).finalize()
    w = U.copy()
    for k in ("para_Pose", "para_SpeedBias", "para_Feature"):
        w[k] = U[k] + s * (P[k] - U[k])
    for i in range(int(w["W"]) + 1):
        q = pose_q(w, i)
        set_pose_q(w, i, q / np.linalg.norm(q))
    return w


def mixed_huber(seed, pre, kw):
    """15 % of the perturbation: the factors fall on both sides of sq = 1.  Two of them get their observation in frame j moved along their own residual so that sq is
    1.005 and 0.995 (an observation is an input of one factor only)"""
    w = blend(seed, pre, 0.15, kw)
    geo = visual_geometry(w)
    order = np.argsort([abs(g["sq"] - 1.0) for g in geo])
    for k, target in ((int(order[0]), 1.005), (int(order[1]), 0.995)):
        r = geo[k]["r"] * np.sqrt(target / geo[k]["sq"])
        td_shift = (w["para_Td"][0] - w["vis_td_j"][k]) * w["vis_vel_j"][2 * k:2 * k + 2]
        w["vis_pts_j"][3 * k:3 * k + 2] = geo[k]["proj"] - r / w["vis_sqrt_info"] + td_shift
    return w


def with_prior(seed, pre, kw):
    """the window after `seed`'s first one, with the oracle's MARGIN_OLD prior of that one (input data, as in tests/golden/ref_window_with_prior)"""
    import synth_window as SW
    w0 = SW.make_window(seed, pre, **kw)
    pre.ba_solve(w0, 4)
    return SW.make_window(seed, pre, frame0=1, prior=pre.ba_marginalize(w0, 0), **kw).finalize()


def sign_flips(w):
    """odd poses stored as -q (the same rotations); the prior's linearisation point gets -q for every other pose-sized block, so that q0^-1 q has w < 0 in all of them"""
    import gfwindow as gw
    for i in range(1, int(w["W"]) + 1, 2):
        set_pose_q(w, i, -pose_q(w, i))
    xo = 0
    for b in w["prior_block_id"]:
        kind, i = int(b) // 4096, int(b) % 4096
        if gw.gsize(kind) == 7 and not (kind == gw.POSE and i % 2 == 1):
            w["prior_x0"][xo + 3:xo + 7] *= -1.0
        xo += gw.gsize(kind)
    return w


def all_fixed(w, flag):
    w["feature_fixed"][:] = flag
    return w


def cut_to_one(w, family, k):
    """the list of one factor family cut to its factor k"""
    if family == "visual":
        tr = tracks_of(w)
        f = int(w["vis_feature"][k])
        q = k - int(np.nonzero(w["vis_feature"] == f)[0][0])
        t = tr[f]
        t["obs"] = [t["obs"][q]]
        t["fixed"] = 0
        return set_tracks(w, [t])
    pre, widths = ("imu_", dict(i=1, sum_dt=1, delta_p=3, delta_q=4, delta_v=3, lin_ba=3, lin_bg=3, jacobian=225, covariance=225)) if family == "imu" else \
                  ("wh_", dict(i=1, sum_dt=1, delta_p=3, delta_q=4, jacobian=18, covariance=36, lin=4, lin_vel=3, lin_gyr=3, vel_1=3, gyr_1=3))
    for key, n in widths.items():
        w[pre + key] = w[pre + key][n * k:n * k + n].copy()
    return w.finalize()


# ---------------------------------------------------------------- the table of cases
# name -> (seed, make_window keywords, builder(window, seed, pre) -> window, kind, solved).  kind "window": H, g, cost at one linearisation; "marg": the MARGIN_OLD prior after four
# iterations.  solved: the case also goes through the eight iterations of the solve (the others are compared at linearisation only: some are ill-conditioned on purpose, a
# solve comparison there would measure the conditioning and not the kernel)
def _plain(edit):
    def make(seed, pre, kw):
        import synth_window as SW
        return edit(SW.make_window(seed, pre, **kw).finalize())
    return make


FREE_TD = dict(fix_td=0)
CASES = {
    "converged": (9, dict(SMALL, perturb=False), _plain(lambda w: w), "window", False),
    "mixed_huber": (41, SMALL, mixed_huber, "window", True),
    "wheel_at_rest": (42, SMALL, _plain(wheel_rest), "window", False),
    "turned": (43, SMALL, _plain(turn), "window", True),
    "sign_flips": (62, MARG, lambda seed, pre, kw: sign_flips(with_prior(seed, pre, kw)), "window", True),
    "td_spread": (45, SMALL, lambda seed, pre, kw: spread_td(_plain(lambda w: w)(seed, pre, kw), seed), "window", True),
    "depth_extremes": (46, MID, _plain(depth_extremes), "window", False),
    "all_fixed": (47, SMALL, _plain(lambda w: all_fixed(w, 1)), "window", False),
    "none_fixed": (47, SMALL, _plain(lambda w: all_fixed(w, 0)), "window", False),
    "track_shapes": (48, MID, _plain(track_shapes), "window", False),
    "imu_bias_far": (49, SMALL, _plain(far_bias), "window", False),
    "wheel_off_lin": (50, SMALL, _plain(lambda w: wheel_off(w, 0.019)), "window", True),
    "wheel_tiny_dtd": (51, SMALL, _plain(lambda w: wheel_off(w, 0.004 + 1e-7)), "window", False),
    # MARGIN_OLD: the window is solved for four iterations first (by whoever makes the fixture; the stored window is the solved one).  Seed 62: the only one of 53 .. 64 (and 44)
    # whose kept system, at 60 digits, has no eigenvalue within a factor 10 of the reference's 1e-8 cut (tests/test_factor_hard_cases_host.py holds the fixtures to that)
    "marg_td_wheel": (52, MARG, lambda seed, pre, kw: wheel_off(spread_td(_plain(lambda w: w)(seed, pre, kw), seed), 0.019), "marg", False),
    "marg_sign_flips": (62, MARG, lambda seed, pre, kw: sign_flips(with_prior(seed, pre, kw)), "marg", False),
    "marg_ten_seconds": (49, SMALL, _plain(far_bias), "marg", False),
}
# the window `turned` is the turned image of (not a case: the metamorphic comparison of the cost needs it)
UNTURNED = (43, SMALL, _plain(lambda w: w), "window", False)


def _single(case, family, pick):
    def make(seed, pre, kw):
        w = CASES[case][2](seed, pre, kw)
        w["fix_td"] = 0
        if family == "wheel":
            w["fix_ix"], w["fix_td_wheel"] = 0, 0
        return cut_to_one(w, family, pick(w))
    return CASES[case][0], CASES[case][1], make, "single", False


def _by_sq(inlier):
    def pick(w):
        sq = np.array([g["sq"] for g in visual_geometry(w)])
        ok = (sq < 0.9) & (sq > 0.05) if inlier else (sq > 1.5)
        return int(np.nonzero(ok)[0][0])
    return pick


def _negative_depth(w):
    return int(np.nonzero(w["para_Feature"][w["vis_feature"]] < 0)[0][1])


# Single-factor windows: one case with the list of one family cut to one factor (the other families stay).  They exist for ONE comparison: each entry of g in the columns
# only that factor feeds against its 60-digit terms, relative to the sum of the absolute terms -- under max |g| of a full window one factor hides.
SINGLES = {
    "one_inlier": _single("converged", "visual", _by_sq(True)),
    "one_outlier": _single("turned", "visual", _by_sq(False)),
    "one_td_shift": _single("td_spread", "visual", lambda w: 7),
    "one_negative_depth": _single("depth_extremes", "visual", _negative_depth),
    "one_far_bias_imu": _single("imu_bias_far", "imu", lambda w: 3),
    "one_off_lin_wheel": _single("wheel_off_lin", "wheel", lambda w: 4),
}
SINGLE_FAMILY = {"one_inlier": "visual", "one_outlier": "visual", "one_td_shift": "visual", "one_negative_depth": "visual", "one_far_bias_imu": "imu", "one_off_lin_wheel": "wheel"}
ALL = dict(CASES, **SINGLES)
WINDOW_CASES = [k for k, v in CASES.items() if v[3] == "window"]
MARG_CASES = [k for k, v in CASES.items() if v[3] == "marg"]
SOLVED_CASES = [k for k, v in CASES.items() if v[4]]
SINGLE_CASES = list(SINGLES)

# the windows the back-end tests had before: seeds of tests/test_backend_gpu.py at make_window's default size, and the windows stored in three 60-digit fixtures
OLD_SEEDS = (1, 2, 3, 4, 6)
OLD_FIXTURES = ("ref_window_free_ex_td", "ref_window_wheel", "ref_window_wheel_free_ix_td")

_made = {}


def window_of(name, pre=None):
    """the case's window (a fresh copy; built once per process).  pre: the pre-integration provider, and for the windows with a prior the solver and marginaliser that make
    the prior (default: the CPU oracle).  name "unturned": the window `turned` is the image of"""
    if name not in _made:
        if pre is None:
            import oracle_py as pre
        seed, kw, make, kind, _ = UNTURNED if name == "unturned" else ALL[name]
        _made[name] = make(seed, pre, kw).finalize()
    return _made[name].copy()


# ---------------------------------------------------------------- the branch decisions, restated
def _rel(x, s):
    return abs(x - s) / s


def _side(counts, key, name):
    counts.setdefault(key, {})
    counts[key][name] = counts[key].get(name, 0) + 1


def census_of(w):
    """counts per switch and side, the smallest distance of any factor from each switch, and the input classes of the window"""
    import gfwindow as gw
    W, NP = int(w["W"]), int(w["W"]) + 1
    c, dist = {}, {}

    def near(key, v):
        dist[key] = min(dist.get(key, np.inf), float(v))

    def exp_side(site, v):          # so3_exp: Taylor below |v|^2 = 1e-20
        t2 = float(v @ v)
        _side(c, "so3_exp(%s)" % site, "taylor" if t2 < 1e-20 else "large")
        near("so3_exp", _rel(t2, 1e-20))

    def rjac_side(site, v):         # rightJacobianSO3: closed form above |v|^2 = 1e-10
        n2 = float(v @ v)
        _side(c, "rightJacobianSO3(%s)" % site, "large" if n2 > 1e-10 else "taylor")
        near("rightJacobianSO3", _rel(n2, 1e-10))

    # ---- visual factors: huber_corrector / vis_lane_eval / vis_lane_cost switch at sq = 1
    geo = visual_geometry(w)
    sq = np.array([g["sq"] for g in geo]) if geo else np.zeros(0)
    z = np.array([g["Xj"][2] for g in geo]) if geo else np.zeros(0)
    td = float(w["para_Td"][0])
    vis = {"factors": len(geo), "outliers": int((sq > 1).sum()), "inliers": int((sq <= 1).sum()), "sq_in_(1,1.01]": int(((sq > 1) & (sq <= 1.01)).sum()),
           "sq_in_[0.99,1)": int(((sq >= 0.99) & (sq < 1)).sum()), "largest_inlier_sq": float("%.4g" % sq[sq <= 1].max()) if (sq <= 1).any() else None,
           "vel_i_zero": int((np.abs(w["vis_vel_i"]).reshape(-1, 2).max(axis=1) == 0).sum()), "td_equals_td_i": int((td - w["vis_td_i"] == 0).sum()),
           "td_equals_td_j": int((td - w["vis_td_j"] == 0).sum()), "td_i_differs_from_td_j": int((w["vis_td_i"] != w["vis_td_j"]).sum()),
           "z_in_camera_j": {"<0": int((z < 0).sum()), "(0.03,0.1)": int(((z > 0.03) & (z < 0.1)).sum()), "[0.1,0.8)": int(((z >= 0.1) & (z < 0.8)).sum()), ">=0.8": int((z >= 0.8).sum())}}
    for v in sq:
        near("huber", abs(v - 1.0))
    for v in z:
        near("z_in_camera_j", abs(v))
    c["visual"] = vis
    dep = w["para_Feature"]
    lengths = {}
    starts = []
    for f in range(int(w["n_feature"])):
        idx = np.nonzero(w["vis_feature"] == f)[0]
        lengths[str(len(idx) + 1)] = lengths.get(str(len(idx) + 1), 0) + 1
        starts.append(int(w["vis_i"][idx[0]]))
    c["features"] = {"features": int(w["n_feature"]), "fixed": int(w["feature_fixed"].sum()), "free_n_e": int((w["feature_fixed"] == 0).sum()),
                     "inverse_depth": {"<0": int((dep < 0).sum()), "(0,0.01]": int(((dep > 0) & (dep <= 0.01)).sum()), "(0.01,1)": int(((dep > 0.01) & (dep < 1)).sum()),
                                       "[1,4)": int(((dep >= 1) & (dep < 4)).sum()), ">=4": int((dep >= 4).sum())},
                     "inverse_depth_range": [float("%.4g" % dep.min()), float("%.4g" % dep.max())] if len(dep) else None,
                     "observations_per_track": dict(sorted(lengths.items(), key=lambda kv: int(kv[0]))), "seen_in_every_frame": lengths.get(str(NP), 0),
                     "starting_at_frame_W-3": int(sum(s == W - 3 for s in starts))}
    # ---- poses
    qs = [pose_q(w, i) for i in range(NP)]
    P = w["para_Pose"].reshape(NP, 7)[:, :3]
    c["poses"] = {"w_negative": int(sum(q[0] < 0 for q in qs)), "w_positive": int(sum(q[0] >= 0 for q in qs)), "smallest_|w|": float("%.4g" % min(abs(q[0]) for q in qs)),
                  "largest_angle_from_identity_deg": float("%.4g" % max(np.degrees(2 * np.arccos(min(1.0, abs(q[0])))) for q in qs)),
                  "sign_changes_between_consecutive": int(sum((qs[i] @ qs[i + 1]) < 0 for i in range(NP - 1))), "largest_|position|_m": float("%.4g" % np.abs(P).max())}
    for q in qs:
        near("pose_w_sign", abs(q[0]))
    # ---- IMU factors
    imu = {"factors": int(w["n_imu"]), "rq_quaternion_w_negative": 0, "sum_dt_under_10": 0, "sum_dt_over_10": 0}
    ratio_p, ratio_v, dba_n, dbg_n = [], [], [], []
    for k in range(int(w["n_imu"])):
        i = int(w["imu_i"][k])
        sbi = w["para_SpeedBias"][9 * i:9 * i + 9]
        J = w["imu_jacobian"][225 * k:225 * k + 225].reshape(15, 15)
        dba, dbg = sbi[3:6] - w["imu_lin_ba"][3 * k:3 * k + 3], sbi[6:9] - w["imu_lin_bg"][3 * k:3 * k + 3]
        cp, cv = J[0:3, 9:12] @ dba + J[0:3, 12:15] @ dbg, J[6:9, 9:12] @ dba + J[6:9, 12:15] @ dbg
        cdp, cdv = w["imu_delta_p"][3 * k:3 * k + 3] + cp, w["imu_delta_v"][3 * k:3 * k + 3] + cv
        ratio_p.append(float(np.max(np.abs(cp) / np.abs(cdp)))); ratio_v.append(float(np.max(np.abs(cv) / np.abs(cdv))))
        dba_n.append(np.linalg.norm(dba)); dbg_n.append(np.linalg.norm(dbg))
        cq = qmul(w["imu_delta_q"][4 * k:4 * k + 4], qexp(J[3:6, 12:15] @ dbg))
        qe = qmul(qinv(cq), qmul(qinv(qs[i]), qs[i + 1]))
        imu["rq_quaternion_w_negative"] += int(qe[0] < 0)
        near("imu_rq_w_sign", abs(qe[0]))
        T = float(w["imu_sum_dt"][k])
        imu["sum_dt_under_10" if T < 10.0 else "sum_dt_over_10"] += 1
        near("sum_dt", _rel(T, 10.0))
    if ratio_p:
        # per factor, the component of corrected_delta_p / corrected_delta_v in which the first-order bias correction is the largest part of the corrected value (gravity fixes the
        # part of the NORM at 0.3 / 9.8 whatever the interval; across the direction of travel and of gravity the correction is what the value consists of)
        imu.update({"|Ba-lin_ba|": float("%.3g" % np.mean(dba_n)), "|Bg-lin_bg|": float("%.3g" % np.mean(dbg_n)),
                    "correction_over_half_of_a_component_of_cdp": int(sum(r > 0.5 for r in ratio_p)), "correction_over_half_of_a_component_of_cdv": int(sum(r > 0.5 for r in ratio_v)),
                    "largest_part_of_a_component_cdp_cdv_median": [float("%.3g" % np.median(ratio_p)), float("%.3g" % np.median(ratio_v))]})
    c["imu"] = imu
    # ---- wheel factors (wheel_factor.h:28-247 restated as far as the switches need)
    wh = {"factors": int(w["n_wheel"]), "lin_off_default": 0, "dtd_nonzero": 0, "dsw_nonzero": 0, "sum_dt_under_10": 0, "sum_dt_over_10": 0}
    if int(w["n_wheel"]):
        qio = pose_q(w, 0, "para_Ex_Pose_wheel")
        sx, sy, sw_ = w["para_Ix"]
        tdw = float(w["para_Td_wheel"][0])
    for k in range(int(w["n_wheel"])):
        i = int(w["wh_i"][k])
        lsx, lsy, lsw, ltd = w["wh_lin"][4 * k:4 * k + 4]
        wh["lin_off_default"] += int((lsx, lsy, lsw, ltd) != (1.0, 1.0, 1.0, 0.0))
        J = w["wh_jacobian"][18 * k:18 * k + 18].reshape(6, 3)
        dq_dsw, dsw, dtd = J[3:6, 2], sw_ - lsw, tdw - ltd
        wh["dtd_nonzero"] += int(dtd != 0); wh["dsw_nonzero"] += int(dsw != 0)
        lin_vel, lin_gyr, vel_1, gyr_1 = (w["wh_" + key][3 * k:3 * k + 3] for key in ("lin_vel", "lin_gyr", "vel_1", "gyr_1"))
        dq0 = w["wh_delta_q"][4 * k:4 * k + 4]
        cq = qmul(dq0 / np.linalg.norm(dq0), qexp(dq_dsw * dsw))
        cq = cq / np.linalg.norm(cq)
        fcw, bcw, fcv = sw_ * lin_gyr * dtd, sw_ * gyr_1 * dtd, np.array([sx, sy, 1.0]) * lin_vel * dtd
        dqt = qmul(qmul(qexp(fcw), cq), qexp(-bcw))
        dqt = dqt / np.linalg.norm(dqt)
        qr = qmul(qmul(qmul(qinv(dqt), qinv(qmul(qs[i], qio))), qs[i + 1]), qio)
        qr = qr / np.linalg.norm(qr)
        rr = qlog(qr)
        exp_side("dq_dsw dsw", dq_dsw * dsw); exp_side("fcw", fcw); exp_side("-bcw", -bcw); exp_side("fcv", fcv); exp_side("-rr", -rr)
        rjac_side("dq_dsw dsw", dq_dsw * dsw); rjac_side("fcw", fcw)
        n2q = float(qr[1:] @ qr[1:])                       # so3_log: Taylor below |vec q|^2 = 1e-20, the pi arm below |w| = 1e-10
        _side(c, "so3_log(rr)", "taylor" if n2q < 1e-20 else "pi" if abs(qr[0]) < 1e-10 else "atan")
        near("so3_log", min(_rel(n2q, 1e-20), _rel(abs(qr[0]), 1e-10)))
        _side(c, "so3_log(rr) w", "negative" if qr[0] < 0 else "positive")
        n2 = float(rr @ rr)                                # rightJacobianInvSO3 of the raw rotation residual
        _side(c, "rightJacobianInvSO3(rr)", "taylor" if n2 <= 1e-10 else "large" if np.sqrt(n2) < np.pi - 1e-5 else "pi")
        _side(c, "rr n2", "<1e-20" if n2 < 1e-20 else "(1e-20,1e-10]" if n2 <= 1e-10 else ">1e-10")
        near("rightJacobianInvSO3", min(_rel(n2, 1e-10), abs(np.sqrt(n2) - (np.pi - 1e-5)) / np.pi))
        T = float(w["wh_sum_dt"][k])
        wh["sum_dt_under_10" if T < 10.0 else "sum_dt_over_10"] += 1
        near("sum_dt", _rel(T, 10.0))
    c["wheel"] = wh
    # ---- MARGIN_OLD reads the sum_dt switch, for the factors of interval 0
    c["margin_old"] = {"imu_kept": int(sum(int(w["imu_i"][k]) == 0 and w["imu_sum_dt"][k] < 10.0 for k in range(int(w["n_imu"])))),
                       "imu_skipped": int(sum(int(w["imu_i"][k]) == 0 and not w["imu_sum_dt"][k] < 10.0 for k in range(int(w["n_imu"])))),
                       "wheel_kept": int(sum(int(w["wh_i"][k]) == 0 and w["wh_sum_dt"][k] < 10.0 for k in range(int(w["n_wheel"])))),
                       "wheel_skipped": int(sum(int(w["wh_i"][k]) == 0 and not w["wh_sum_dt"][k] < 10.0 for k in range(int(w["n_wheel"]))))}
    # ---- prior_block_dx: the sign of (q0^-1 q).w per pose-sized block
    pr = {"columns": int(w["prior_n"]), "pose_sized_blocks": 0, "dq_w_negative": 0, "dq_w_negative_poses": 0, "poses": 0}
    xo = 0
    for b in w["prior_block_id"]:
        kind, i = int(b) // 4096, int(b) % 4096
        if gw.gsize(kind) == 7:
            x0 = w["prior_x0"][xo:xo + 7]
            q = pose_q(w, i) if kind == gw.POSE else pose_q(w, 0, "para_Ex_Pose" if kind == gw.EX_POSE else "para_Ex_Pose_wheel")
            dq = qmul(qinv(np.array([x0[6], x0[3], x0[4], x0[5]])), q)
            pr["pose_sized_blocks"] += 1; pr["dq_w_negative"] += int(dq[0] < 0)
            pr["poses"] += int(kind == gw.POSE); pr["dq_w_negative_poses"] += int(kind == gw.POSE and dq[0] < 0)
            near("prior_dq_w_sign", abs(dq[0]))
        xo += gw.gsize(kind)
    c["prior"] = pr
    c["fixed_blocks"] = {k: int(w[k]) for k in ("fix_ex_pose", "fix_ex_wheel", "fix_ix", "fix_td", "fix_td_wheel")}
    c["smallest_distance_from_switch"] = {k: float("%.4g" % v) for k, v in sorted(dist.items())}
    return c


def old_inputs(pre):
    import synth_window as SW
    import gfwindow as gw
    out = {}
    for s in OLD_SEEDS:
        out["seed_%d" % s] = SW.make_window(s, pre).finalize()
    for name in OLD_FIXTURES:
        with gzip.open(os.path.join(HERE, "golden", name + ".json.gz"), "rt") as f:
            fx = json.load(f)
        w = gw.Window()
        for k, v in fx["window"].items():
            w[k] = np.array(v) if isinstance(v, list) else v
        out[name] = w.finalize()
    return out


def census_document(pre=None, measured=None):
    """the file profiles/factor_hard_census.json.  measured: the oracle's distance from each new 60-digit fixture, which only the fixture generator computes
    (tests/golden/make_ref_golden.py factor_hard writes it when it writes the fixture); recomputing the census carries that block over from the committed file unchanged"""
    if pre is None:
        import oracle_py as pre
    doc = {"about": "branch and input-class census of the visual, IMU and wheel factors (tests/factor_hard_cases.py census_of): per window, how many factors take each side of "
                    "each switch, the smallest distance of a factor from each switch, the classes of the inputs",
           "margin_required": MARGIN, "cases": {k: census_of(window_of(k, pre)) for k in CASES}, "single_factor_windows": {k: census_of(window_of(k, pre)) for k in SINGLES},
           "unturned": census_of(window_of("unturned", pre)), "inputs_before": {k: census_of(w) for k, w in old_inputs(pre).items()}}
    doc["measured"] = measured if measured is not None else committed().get("measured", {})
    return doc


CENSUS_PATH = os.path.join(ROOT, "profiles", "factor_hard_census.json")


def committed():
    if not os.path.exists(CENSUS_PATH):
        return {}
    with open(CENSUS_PATH) as f:
        return json.load(f)


def write(doc):
    with open(CENSUS_PATH, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


# ---------------------------------------------------------------- the bars against 60 digits (see tests/test_factor_hard_cases_host.py)
def measured_of(name):
    return committed()["measured"]["oracle_vs_60_digits"][name]


def tol_of(name):
    m = measured_of(name)
    worst = max(m["oracle_cost_rel"], m["oracle_H_scaled"], m["oracle_g_rel"])
    return 1e-11 if worst < 2.5e-12 else 4 * worst


def own_columns_tol_of(name):
    worst = measured_of(name)["oracle_g_own_columns_rel_abs_sum"]
    return 1e-11 if worst < 2.5e-12 else 4 * worst


if __name__ == "__main__":
    doc = census_document()
    write(doc)
    for group in ("cases", "single_factor_windows", "inputs_before"):
        for name, c in doc[group].items():
            print(name, "visual %d out / %d in" % (c["visual"]["outliers"], c["visual"]["inliers"]), "poses w<0:", c["poses"]["w_negative"], c["smallest_distance_from_switch"])
