"""tests/golden/camera_models.json.gz: liftProjective of camodocal's MEI and KANNALA_BRANDT cameras at 60 digits (python tests/golden/make_camera_golden.py;
the fixture is described in tests/golden/README_camera_models.md).

Transcribed into mpmath, line by cited line, from the reference (nothing shared with the library):
  CataCamera::liftProjective          camera_models/src/camera_models/CataCamera.cc:556-626 (the recursive distortion branch), distortion :766-782
  EquidistantCamera::liftProjective   EquidistantCamera.cc:428-442, backprojectSymmetric :716-818 (roots by mpmath.polyroots, the reference's 1e-10 tolerances)
  the caller's float pair             feature_tracker.cpp:803-805: (float)(P.x / P.z), (float)(P.y / P.z)
Calibrations are synthetic and named.  Points per calibration: the principal point, a point 1e-12 px from it (double only: no float pixel lies there), the four
corners of 640 x 480 and 60 seeded float pixels; a seeded point within 1e-6 of a turning value of r(theta) is drawn again (the root is ill-conditioned there and
the reference's own answer is noise).  Every expected value is stored as a pair of doubles (hi, lo), hi + lo = the 60-digit value to ~1e-25 of it.

eps_d, the bar of the tests: the error of the reference's OWN route in double precision -- numpy.roots on the same polynomial with the same tolerances, sin / cos /
atan2 / sqrt in IEEE double -- against the 60-digit rays over all these points, as |got - exact| / max(1, |exact|) per component; the fixture stores the largest
(`ref_route_max_err`) and four times it (`eps_d`).
"""
import gzip
import json
import math
import os

import mpmath as mp
import numpy as np

mp.mp.dps = 60
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "camera_models.json.gz")
W, H = 640, 480
PINHOLE, MEI, KB = 0, 1, 2
TOL = mp.mpf("1e-10")

# proj: gamma1 gamma2 u0 v0 | mu mv u0 v0 (all exactly representable as float, so the principal point is a float pixel); dist: k1 k2 p1 p2 | k2 k3 k4 k5
CASES = [
    ("mei_xi1", MEI, [470.5, 468.25, 320.5, 240.25], [-0.02, 0.003, 2e-4, -1e-4], 1.0),
    ("mei_xi199_dist", MEI, [905.5, 903.75, 318.25, 242.5], [-0.015, 0.002, -1.5e-4, 2.5e-4], 1.99),
    ("mei_xi07_nodist", MEI, [610.25, 612.5, 322.75, 238.5], [0.0, 0.0, 0.0, 0.0], 0.7),
    ("mei_xi0_dist", MEI, [520.5, 522.25, 321.25, 239.75], [-0.02, 0.003, 2e-4, -1e-4], 0.0),
    ("kb_zero", KB, [285.5, 286.25, 320.5, 240.25], [0.0, 0.0, 0.0, 0.0], 0.0),
    ("kb_k2", KB, [285.5, 286.25, 320.5, 240.25], [-0.03, 0.0, 0.0, 0.0], 0.0),
    ("kb_k2k3", KB, [285.5, 286.25, 320.5, 240.25], [-0.02, 0.008, 0.0, 0.0], 0.0),
    ("kb_k2k3k4", KB, [285.5, 286.25, 320.5, 240.25], [-0.015, 0.007, -0.002, 0.0], 0.0),
    ("kb_mono9", KB, [285.5, 286.25, 320.5, 240.25], [-0.012, 0.006, -0.003, 0.0006], 0.0),
    ("kb_neglead", KB, [285.5, 286.25, 320.5, 240.25], [0.02, -0.01, 0.004, -0.05], 0.0),
    ("kb_wiggle", KB, [285.5, 286.25, 320.5, 240.25], [-0.9, 0.35, -0.05, 0.0025], 0.0),
]


def f32(x):
    return float(np.float32(x))


def hilo(x):
    hi = float(x)
    return [hi, float("%.8e" % float(x - mp.mpf(hi)))]   # lo to nine digits: hi + lo is the value to ~1e-25 of it


def mei_distortion(k1, k2, p1, p2, x, y):   # CataCamera.cc:766-782
    mx2, my2, mxy = x * x, y * y, x * y
    rho2 = mx2 + my2
    rad = k1 * rho2 + k2 * rho2 * rho2
    return (x * rad + 2 * p1 * mxy + p2 * (rho2 + 2 * mx2), y * rad + 2 * p2 * mxy + p1 * (rho2 + 2 * my2))


def mei_lift(proj, dist, xi, u, v, F=mp.mpf, sqrt=mp.sqrt):   # CataCamera.cc:556-626
    g1, g2, u0, v0 = [F(t) for t in proj]
    k1, k2, p1, p2 = [F(t) for t in dist]
    xi = F(xi)
    mx_d = (1 / g1) * F(u) + (-u0 / g1)   # m_inv_K11 * p(0) + m_inv_K13, CataCamera.cc:320-323, :563-564
    my_d = (1 / g2) * F(v) + (-v0 / g2)
    if k1 == 0 and k2 == 0 and p1 == 0 and p2 == 0:   # m_noDistortion, :306-317
        mx_u, my_u = mx_d, my_d
    else:
        dx, dy = mei_distortion(k1, k2, p1, p2, mx_d, my_d)   # :598-610, n = 8
        mx_u, my_u = mx_d - dx, my_d - dy
        for _ in range(1, 8):
            dx, dy = mei_distortion(k1, k2, p1, p2, mx_u, my_u)
            mx_u, my_u = mx_d - dx, my_d - dy
    if xi == 1:   # :616-619
        return [mx_u, my_u, (1 - mx_u * mx_u - my_u * my_u) / 2]
    rho2 = mx_u * mx_u + my_u * my_u   # :623-624
    return [mx_u, my_u, 1 - xi * (rho2 + 1) / (xi + sqrt(1 + (1 - xi * xi) * rho2))]


def kb_coeffs(dist, rho):   # EquidistantCamera.cc:731-769: npow by the NUMBER of zero coefficients (the sets here have them at the end)
    npow = 9 - 2 * sum(1 for k in dist if k == 0.0)
    c = [0] * (npow + 1)
    c[0], c[1] = -rho, 1
    for j, p in enumerate((3, 5, 7, 9)):
        if npow >= p:
            c[p] = dist[j]
    return npow, c


def kb_roots_mp(dist, rho):
    """the non-negative real roots backprojectSymmetric keeps (EquidistantCamera.cc:787-807), ascending"""
    npow, c = kb_coeffs([mp.mpf(k) for k in dist], rho)
    if npow == 1:
        return None
    roots = mp.polyroots(list(reversed(c)), maxsteps=500, extraprec=400)
    keep = []
    for z in roots:
        if abs(mp.im(z)) > TOL:
            continue
        t = mp.re(z)
        if t < -TOL:
            continue
        keep.append(mp.mpf(0) if t < 0 else t)
    return sorted(keep)


def kb_lift(proj, dist, u, v):   # EquidistantCamera.cc:428-442, :716-818
    mu, mv, u0, v0 = [mp.mpf(t) for t in proj]
    px = (1 / mu) * mp.mpf(u) + (-u0 / mu)
    py = (1 / mv) * mp.mpf(v) + (-v0 / mv)
    rho = mp.sqrt(px * px + py * py)
    phi = mp.mpf(0) if rho < TOL else mp.atan2(py, px)
    roots = kb_roots_mp(dist, rho)
    if roots is None:
        theta, nroots = rho, 1
    elif not roots:
        theta, nroots = rho, 0
    else:
        theta, nroots = roots[0], len(roots)
    return [mp.sin(theta) * mp.cos(phi), mp.sin(theta) * mp.sin(phi), mp.cos(theta)], rho, theta, nroots


def kb_lift_double(proj, dist, u, v):
    """the same route in IEEE double with numpy.roots: what the reference computes, for eps_d"""
    mu, mv, u0, v0 = proj
    px = (1.0 / mu) * u + (-u0 / mu)
    py = (1.0 / mv) * v + (-v0 / mv)
    rho = math.sqrt(px * px + py * py)
    phi = 0.0 if rho < 1e-10 else math.atan2(py, px)
    npow, c = kb_coeffs(dist, rho)
    if npow == 1:
        theta = rho
    else:
        keep = []
        for z in np.roots(list(reversed(c))):
            if abs(z.imag) > 1e-10 or z.real < -1e-10:
                continue
            keep.append(max(z.real, 0.0))
        theta = min(keep) if keep else rho
    return [math.sin(theta) * math.cos(phi), math.sin(theta) * math.sin(phi), math.cos(theta)]


def kb_turning(dist):
    """turning points of r(theta) in theta > 0: the positive real roots of r'(theta) = 1 + 3 k2 s + 5 k3 s^2 + 7 k4 s^3 + 9 k5 s^4, s = theta^2 (all simple here)"""
    q = [mp.mpf(1), 3 * mp.mpf(dist[0]), 5 * mp.mpf(dist[1]), 7 * mp.mpf(dist[2]), 9 * mp.mpf(dist[3])]
    while len(q) > 1 and q[-1] == 0:
        q.pop()
    if len(q) == 1:
        return []
    out = []
    for z in mp.polyroots(list(reversed(q)), maxsteps=500, extraprec=400):
        if abs(mp.im(z)) < mp.mpf("1e-40") and mp.re(z) > 0:
            t = mp.sqrt(mp.re(z))
            k2, k3, k4, k5 = [mp.mpf(k) for k in dist]
            out.append((t, t + k2 * t ** 3 + k3 * t ** 5 + k4 * t ** 7 + k5 * t ** 9))
    return sorted(out)


def build_case(name, model, proj, dist, xi, rng):
    turning = kb_turning(dist) if model == KB else []
    points, worst = [], mp.mpf(0)

    def add(u, v, double_only, seeded):
        nonlocal worst
        if model == MEI:
            P = mei_lift(proj, dist, xi, u, v)
            Pd = mei_lift(proj, dist, xi, u, v, F=float, sqrt=math.sqrt)
            rho = theta = None
            nroots = 1
            switch = {"xi_minus_1": float(mp.mpf(xi) - 1)}
        else:
            P, rho, theta, nroots = kb_lift(proj, dist, u, v)
            Pd = kb_lift_double(proj, dist, u, v)
            near = [abs(rho - r) for _, r in turning]
            if seeded and near and min(near) < mp.mpf("1e-6"):
                return False
            switch = {"rho_minus_1e-10": float("%.6e" % float(rho - TOL)), "rho_minus_turning": [float("%.6e" % float(rho - r)) for _, r in turning]}
        norm = mp.sqrt(P[0] ** 2 + P[1] ** 2 + P[2] ** 2)
        for a, b in zip(Pd, P):
            worst = max(worst, abs(mp.mpf(a) - b) / max(1, abs(b)))
        pair_ok = bool(abs(P[2]) / norm >= mp.mpf("0.05"))
        pt = {"uv": [u, v], "double_only": double_only, "ray": [hilo(t) for t in P], "pair_ok": pair_ok, "n_roots": nroots, "switch": switch}
        if pair_ok:
            pt["un"] = [hilo(P[0] / P[2]), hilo(P[1] / P[2])]
        if rho is not None:
            pt["rho"], pt["theta"] = float(rho), float(theta)
        points.append(pt)
        return True

    u0, v0 = proj[2], proj[3]
    add(u0, v0, False, False)
    add(u0 + 1e-12 * proj[0] * 0.6, v0 + 1e-12 * proj[1] * 0.8, True, False)   # |p_u| = 1e-12 < 1e-10: the phi = 0 branch
    for u, v in ((0.0, 0.0), (W - 1.0, 0.0), (0.0, H - 1.0), (W - 1.0, H - 1.0)):
        add(u, v, False, False)
    n = 0
    while n < 60:
        u, v = f32(rng.uniform(0, W - 1)), f32(rng.uniform(0, H - 1))
        if add(u, v, False, True):
            n += 1
    by_ray_only = sum(1 for p in points if not p["pair_ok"])
    assert by_ray_only <= 0.05 * len(points), (name, by_ray_only)
    case = {"name": name, "model": model, "proj": proj, "dist": dist, "xi": xi, "turning": [[hilo(t), hilo(r)] for t, r in turning], "points": points}
    return case, worst


def main():
    rng = np.random.default_rng(20240917)
    cases, worst = [], mp.mpf(0)
    for name, model, proj, dist, xi in CASES:
        case, w = build_case(name, model, proj, dist, xi, rng)
        regimes = sorted({p["n_roots"] for p in case["points"]})
        print("%-16s %d points, turning %s, numbers of kept roots %s, by ray only %d, reference route in double: %.3g" % (
            name, len(case["points"]), [(round(t[0], 4), round(r[0], 4)) for t, r in case["turning"]], regimes,
            sum(1 for p in case["points"] if not p["pair_ok"]), float(w)))
        cases.append(case)
        worst = max(worst, w)
    doc = {"what": "liftProjective of camodocal's MEI and KANNALA_BRANDT cameras at 60 digits; see tests/golden/make_camera_golden.py",
           "image": [W, H], "ref_route_max_err": float(worst), "eps_d": float(4 * worst), "cases": cases}
    with gzip.GzipFile(OUT, "wb", mtime=0) as f:
        f.write(json.dumps(doc, separators=(",", ":")).encode())
    print("eps_d = %.3g (4 x %.3g) -> %s, %d bytes" % (doc["eps_d"], doc["ref_route_max_err"], OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
