"""tests/golden/camera_models_wide.json.gz: liftProjective and spaceToPlane of camodocal's PINHOLE_FULL and SCARAMUZZA cameras (python
tests/golden/make_camera_wide_golden.py; the fixture is described in tests/golden/README_camera_models_wide.md, which this script writes too).

Transcribed line by cited line from the reference, twice, with nothing shared with the library:
  PinholeFullCamera::liftProjective   camera_models/src/camera_models/PinholeFullCamera.cc:535-607
  PinholeFullCamera::spaceToPlane     :623-645 with distortion :754-780
  OCAMCamera::liftProjective          ScaramuzzaCamera.cc:599-622 (m_inv_scale :200)
  OCAMCamera::spaceToPlane            :632-655
  the caller's float pair             feature_tracker.cpp:803-805: (float)(P.x / P.z), (float)(P.y / P.z)
once in mpmath at 60 digits (`F = mp.mpf`) and once in numpy float64 scalars in the reference's order of operations (`F = np.float64`): what the reference's
binary computes, stored exactly as hex.

The DEFINITION of PINHOLE_FULL's lift is the reference's loop as it runs: `int min_error = 0.01` is 0, `error` comes from xd, yd that are
never assigned and no distance is < 0, so the loop ends on `j > max_cnt` alone -- nine passes, j = 0 .. 8, no error test, no re-projection.  The ninth iterate is
not the true inverse; `inv_dist` stores how far it is from it (Newton at 60 digits on the forward distortion, from the iterate), as information.

Per camera and point:
  uv                 the pixel (float32-representable: the device lifts float pixels), hex
  ray_d, un_d, px_d  numpy float64: the ray, the float pair, and spaceToPlane OF ray_d; hex ("nan", "inf" where they are)
  ray60, px60        60 digits as (hi, lo) pairs of doubles: the ray of uv and spaceToPlane of the DOUBLES ray_d; null where a value is not finite
  inv_dist           PINHOLE_FULL: |ninth iterate - true inverse| on the normalised plane, null where Newton found none
`sca_proj_route_max_err`: the largest |px_d - px60| / max(1, |px60|) over the SCARAMUZZA points, the error of the reference's own double route through atan2;
the tests' bar for that projection is four times it.
"""
import gzip
import json
import math
import os

import mpmath as mp
import numpy as np

mp.mp.dps = 60
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "camera_models_wide.json.gz")
README = os.path.join(HERE, "README_camera_models_wide.md")
W, H = 640, 480
FULL, SCA = 3, 4
FULL_PASSES = 9


def fisheye_polys(f, r_max):
    """OCamCalib polynomials of an ideal equidistant fisheye r = f theta (theta from the axis): z(phi) = -phi / tan(phi / f), the ray being (x, y, -z), by least
    squares on 1 .. r_max pixels; and its inverse rho(theta'), theta' = atan2(z, phi), of degree 11.  Rounded to 12 digits: a calibration file's precision."""
    phi = np.linspace(1.0, r_max, 400)
    z = -phi / np.tan(phi / f)
    poly = np.polynomial.polynomial.polyfit(phi, z, 4)
    th = np.arctan2(np.polynomial.polynomial.polyval(phi, poly), phi)
    inv = np.polynomial.polynomial.polyfit(th, phi, 11)
    r12 = lambda v: float("%.12e" % v)
    return [r12(v) for v in poly], [r12(v) for v in inv] + [0.0] * 8


# proj fx fy cx cy and dist k1 k2 p1 p2 k3 k4 k5 k6; focal lengths and centres exactly representable as float
FULL_CASES = [
    ("full_zero", [520.5, 522.25, 321.25, 239.75], [0.0] * 8),
    ("full_opencv5", [520.5, 522.25, 321.25, 239.75], [-0.28, 0.09, 2e-4, -1e-4, -0.015, 0.0, 0.0, 0.0]),             # k1 k2 p1 p2 k3 of calibrateCamera
    ("full_kinect8", [504.5, 504.75, 322.5, 241.25], [0.52, -2.7, 4e-4, -1.5e-4, 1.5, 0.4, -2.5, 1.4]),               # CALIB_RATIONAL_MODEL, Kinect-class magnitudes
    ("full_barrel", [400.0, 400.0, 320.0, 240.0], [-0.25, 0.05, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]),                        # the fixed point converges slowly at the corner
    ("full_pole", [256.0, 256.0, 320.0, 240.0], [-1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]),                            # 1 + k1 r2 = 0 on the circle r = 1: 256 px from the centre
]
P190, I190 = fisheye_polys(240.0, 420.0)   # 95 degrees at the corner of 640 x 480 (398.6 px from the centre)
P228, I228 = fisheye_polys(145.0, 300.0)   # the horizon 228 px from the centre: inside the image
SCA_CASES = [
    ("sca_190_identity", P190, I190, [1.0, 0.0, 0.0, 320.0, 240.0]),
    ("sca_affine", P190, I190, [1.0005, 2e-4, -3e-4, 318.5, 241.25]),
    ("sca_horizon_inside", P228, I228, [1.0, 0.0, 0.0, 320.0, 240.0]),
]
# the centre pixel, the four corners, pixels well outside the image, NaN and both infinities; then seeded pixels of the image
FIXED_POINTS = [(320.0, 240.0), (0.0, 0.0), (W - 1.0, 0.0), (0.0, H - 1.0), (W - 1.0, H - 1.0), (-2000.0, -1500.0), (5000.0, 4000.0), (1e6, -1e6),
                (math.nan, 100.0), (100.0, math.nan), (math.inf, 100.0), (100.0, -math.inf), (-math.inf, math.inf)]
EXTRA_POINTS = {"full_pole": [(576.0, 240.0), (320.0, 496.0)]}   # on the circle: r2 == 1 exactly in the first pass, 1 / 0
N_SEEDED = 20


def full_lift(proj, dist, u, v, F):   # PinholeFullCamera.cc:535-607
    fx, fy, cx, cy = [F(t) for t in proj]
    k1, k2, p1, p2, k3, k4, k5, k6 = [F(t) for t in dist]   # :537-544
    ifx, ify = 1 / fx, 1 / fy                               # :548-549
    mx_d = ifx * F(u) + (-cx / fx)                          # :554, m_inv_K13 :375
    my_d = ify * F(v) + (-cy / fy)                          # :555, m_inv_K23 :377
    x, y = mx_d, my_d                                       # :558-559
    x0, y0 = x, y                                           # :560-561
    for _ in range(FULL_PASSES):                            # :567-570, j = 0 .. 8
        r2 = x * x + y * y                                                                                  # :574
        icdist = (1 + ((k6 * r2 + k5) * r2 + k4) * r2) / (1 + ((k3 * r2 + k2) * r2 + k1) * r2)              # :575-576
        deltaX = 2 * p1 * x * y + p2 * (r2 + 2 * x * x)                                                     # :577
        deltaY = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y                                                     # :578
        x = (x0 - deltaX) * icdist                                                                          # :580
        y = (y0 - deltaY) * icdist                                                                          # :581
    return [x, y, F(1)], (mx_d, my_d)                       # :606


def full_distort(dist, x, y, F):   # PinholeFullCamera.cc:754-780: d_u
    k1, k2, p1, p2, k3, k4, k5, k6 = [F(t) for t in dist]
    r2 = x * x + y * y                                      # :770
    r4 = r2 * r2                                            # :771
    r6 = r4 * r2                                            # :772
    a1 = 2 * x * y                                          # :773
    a2 = r2 + 2 * x * x                                     # :774
    a3 = r2 + 2 * y * y                                     # :775
    cdist = 1 + k1 * r2 + k2 * r4 + k3 * r6                 # :776
    icdist2 = 1 / (1 + k4 * r2 + k5 * r4 + k6 * r6)         # :777
    return (x * cdist * icdist2 + p1 * a1 + p2 * a2 - x,    # :779
            y * cdist * icdist2 + p1 * a3 + p2 * a1 - y)    # :780


def full_project(proj, dist, P, F):   # PinholeFullCamera.cc:623-645; the m_noDistortion branch (:630-633) is the same value
    fx, fy, cx, cy = [F(t) for t in proj]
    xu, yu = P[0] / P[2], P[1] / P[2]                       # :628
    dx, dy = full_distort(dist, xu, yu, F)                  # :638
    xd, yd = xu + dx, yu + dy                               # :639
    return [fx * xd + cx, fy * yd + cy]                     # :643-644


def sca_lift(poly, affine, u, v, F, sqrt):   # ScaramuzzaCamera.cc:599-622
    ac, ad, ae, cx, cy = [F(t) for t in affine]
    inv_scale = 1 / (ac - ad * ae)                          # :200
    xc0, xc1 = F(u) - cx, F(v) - cy                         # :602
    xa0 = inv_scale * (xc0 - ad * xc1)                      # :607
    xa1 = inv_scale * (-ae * xc0 + ac * xc1)                # :608
    phi = sqrt(xa0 * xa0 + xa1 * xa1)                       # :611
    phi_i, z = F(1), F(0)                                   # :612-613
    for i in range(5):                                      # :615-619
        z += phi_i * F(poly[i])
        phi_i *= phi
    return [xc0, xc1, -z], (xa0, xa1)                       # :621: the UNCORRECTED xc


def sca_project(inv_poly, affine, P, F, sqrt, atan2):   # ScaramuzzaCamera.cc:632-655
    ac, ad, ae, cx, cy = [F(t) for t in affine]
    norm = sqrt(P[0] * P[0] + P[1] * P[1])                  # :634
    theta = atan2(-P[2], norm)                              # :635
    rho, theta_i = F(0), F(1)                               # :636-637
    for i in range(20):                                     # :639-643
        rho += theta_i * F(inv_poly[i])
        theta_i *= theta
    invNorm = 1 / norm                                      # :645
    xn0, xn1 = P[0] * invNorm * rho, P[1] * invNorm * rho   # :646-649
    return [xn0 * ac + xn1 * ad + cx, xn0 * ae + xn1 + cy]  # :651-652


D = np.float64
hx = lambda v: float(v).hex()


def hilo(x):
    hi = float(x)
    return [hx(hi), hx(float("%.8e" % float(x - mp.mpf(hi))))]


def at60(fn):
    """fn() at 60 digits -> list of (hi, lo), or None where a value is not finite (mpmath raises on x / 0)"""
    try:
        vals = fn()
    except ZeroDivisionError:
        return None
    if not all(mp.isfinite(t) for t in vals):
        return None
    return [hilo(t) for t in vals]


def true_inverse(dist, target, start):
    """(x, y) with (x, y) + d_u(x, y) = target at 60 digits, by Newton from `start`; None without convergence"""
    f = lambda x, y: [x + full_distort(dist, x, y, mp.mpf)[0] - target[0], y + full_distort(dist, x, y, mp.mpf)[1] - target[1]]
    try:
        r = mp.findroot(f, start, tol=mp.mpf("1e-50"), maxsteps=200)
        return r[0], r[1]
    except (ValueError, ZeroDivisionError):
        return None


def build_point(model, case, u, v):
    finite_in = math.isfinite(u) and math.isfinite(v)
    pt = {"uv": [hx(u), hx(v)]}
    with np.errstate(all="ignore"):
        if model == FULL:
            _, proj, dist = case
            ray_d, _ = full_lift(proj, dist, u, v, D)
            px_d = full_project(proj, dist, ray_d, D)
        else:
            _, poly, inv_poly, affine = case
            ray_d, _ = sca_lift(poly, affine, u, v, D, np.sqrt)
            px_d = sca_project(inv_poly, affine, ray_d, D, np.sqrt, np.arctan2)
        un_d = [np.float32(ray_d[0] / ray_d[2]), np.float32(ray_d[1] / ray_d[2])]   # feature_tracker.cpp:803-805
    pt["ray_d"], pt["un_d"], pt["px_d"] = [hx(t) for t in ray_d], [hx(t) for t in un_d], [hx(t) for t in px_d]
    ray_in = [mp.mpf(float(t)) for t in ray_d]
    if model == FULL:
        pt["ray60"] = at60(lambda: full_lift(proj, dist, u, v, mp.mpf)[0]) if finite_in else None
        pt["px60"] = at60(lambda: full_project(proj, dist, ray_in, mp.mpf)) if all(math.isfinite(t) for t in ray_d) else None
        pt["inv_dist"] = None
        if pt["ray60"]:
            P, target = full_lift(proj, dist, u, v, mp.mpf)
            inv = true_inverse(dist, target, (P[0], P[1]))
            if inv:
                pt["inv_dist"] = float("%.6e" % float(mp.sqrt((P[0] - inv[0]) ** 2 + (P[1] - inv[1]) ** 2)))
    else:
        pt["ray60"] = at60(lambda: sca_lift(poly, affine, u, v, mp.mpf, mp.sqrt)[0]) if finite_in else None
        pt["px60"] = at60(lambda: sca_project(inv_poly, affine, ray_in, mp.mpf, mp.sqrt, mp.atan2)) if all(math.isfinite(t) for t in ray_d) else None
    return pt


def value60(hl):
    return mp.mpf(float.fromhex(hl[0])) + mp.mpf(float.fromhex(hl[1]))


def main():
    rng = np.random.default_rng(20241020)
    seeded = [(float(np.float32(rng.uniform(0, W - 1))), float(np.float32(rng.uniform(0, H - 1)))) for _ in range(N_SEEDED)]
    cases, sca_worst, lines = [], mp.mpf(0), []
    for model, group in ((FULL, FULL_CASES), (SCA, SCA_CASES)):
        for case in group:
            name = case[0]
            pts = [build_point(model, case, u, v) for u, v in FIXED_POINTS + EXTRA_POINTS.get(name, []) + seeded]
            doc = {"name": name, "model": model, "points": pts}
            if model == FULL:
                doc["proj"], doc["dist"] = case[1], case[2]
                inside = lambda p: all(0 <= float.fromhex(t) <= m for t, m in zip(p["uv"], (W - 1, H - 1)))
                far = [p["inv_dist"] for p in pts if p["inv_dist"] is not None and inside(p)]
                lines.append("| `%s` | %d | %d | ninth iterate from the true inverse, pixels of the image: at most %.3g, at the corner (639, 479) %s |" % (
                    name, len(pts), sum(1 for p in pts if not all(math.isfinite(float.fromhex(t)) for t in p["ray_d"])), max(far), pts[4]["inv_dist"]))
            else:
                doc["poly"], doc["inv_poly"], doc["affine"] = case[1], case[2], case[3]
                worst = mp.mpf(0)
                for p in pts:
                    if p["px60"]:
                        for got, want in zip(p["px_d"], p["px60"]):
                            w = value60(want)
                            worst = max(worst, abs(mp.mpf(float.fromhex(got)) - w) / max(1, abs(w)))
                sca_worst = max(sca_worst, worst)
                lines.append("| `%s` | %d | %d | projection by the double route from 60 digits: at most %.3g of max(1, pixel) |" % (
                    name, len(pts), sum(1 for p in pts if not all(math.isfinite(float.fromhex(t)) for t in p["ray_d"])), float(worst)))
            cases.append(doc)
            print(lines[-1])
    out = {"what": "liftProjective and spaceToPlane of camodocal's PINHOLE_FULL and SCARAMUZZA cameras; see tests/golden/make_camera_wide_golden.py",
           "image": [W, H], "full_passes": FULL_PASSES, "n_fixed": len(FIXED_POINTS), "n_seeded": N_SEEDED, "sca_proj_route_max_err": float(sca_worst), "cases": cases}
    with gzip.GzipFile(OUT, "wb", mtime=0) as f:
        f.write(json.dumps(out, separators=(",", ":")).encode())
    with open(README, "w") as f:
        f.write("# camera_models_wide.json.gz\n\nWritten by `python tests/golden/make_camera_wide_golden.py` (mpmath at 60 digits and numpy float64; its docstring has the layout and the\n"
                "reference lines every expression transcribes).  Read by `tests/test_camera_wide_host.py`, `tests/native/camera_wide_host.cpp` and\n`tests/test_camera_wide_gpu.py`.\n\n"
                "%d fixed points per camera -- the centre pixel, the four corners of %d x %d, three pixels well outside the image, NaN and both infinities --\n"
                "then the camera's own extra points and %d seeded float pixels of the image.\n\n"
                "| camera | points | with a non-finite ray | measured |\n|---|---|---|---|\n%s\n\n"
                "PINHOLE_FULL's lift is defined as the reference's loop as it runs, nine passes without an error test: the ninth iterate, not the true inverse.  The\n"
                "last column shows how far apart the two are; for `full_barrel` the corner is still more than 1e-6 away.  `full_pole` has 1 + k1 r^2 = 0 on a circle\n"
                "inside the image; the two extra points lie on it exactly and come out non-finite after bounded work.\n\n"
                "Both lifts and PINHOLE_FULL's projection involve no transcendental: the tests ask for the bits of the numpy float64 route.  SCARAMUZZA's projection\n"
                "goes through atan2: the numpy double route deviates from the 60-digit value by at most **%.3g** of max(1, |pixel|) over the fixture\n"
                "(`sca_proj_route_max_err`); the tests' bar is four times that, %.3g.\n" % (
                    len(FIXED_POINTS), W, H, N_SEEDED, "\n".join(lines), float(sca_worst), float(4 * sca_worst)))
    print("sca_proj_route_max_err = %.3g -> %s, %d bytes" % (float(sca_worst), OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
