// gf_camera_models.hpp — the camera models of camodocal that the reference's front end can be given (CameraFactory::generateCameraFromYamlFile through
// FeatureTracker::readIntrinsicParameter, feature_tracker.cpp:745-759): liftProjective and spaceToPlane of
//   PINHOLE          PinholeCamera.cc:450-510, :520-542, :646-662
//   MEI              CataCamera.cc:556-626 (the recursive distortion branch; `xi == 1.0` apart), :636-659, distortion :766-782
//   KANNALA_BRANDT   EquidistantCamera.cc:428-442 with backprojectSymmetric :716-818, spaceToPlane :451-461, r() EquidistantCamera.h:160-168
//   PINHOLE_FULL     PinholeFullCamera.cc:535-607 (nine passes, no error test: see full_lift), :623-645, distortion :754-780
//   SCARAMUZZA       ScaramuzzaCamera.cc:599-622, :632-655 (a ray on the axis projects to a non-finite pixel, as there: see scaramuzza_to_plane)
// in double precision.  Plain C++ that host and device both compile: one source for the tracker's host bookkeeping (gf_track_host.hpp), the lift kernel
// (gf_camera_kernels.hpp) and the stand-alone host program of the tests (tests/native/camera_models_host.cpp).  It sets no floating-point contraction of its own;
// the library compiles it without contraction on both sides, so the arithmetic (everything but sin / cos / atan2 / acos) gives the same bits there.
//
// backprojectSymmetric finds theta as the smallest non-negative real eigenvalue of the companion matrix of theta + k2 theta^3 + .. + k5 theta^9 - |p_u|, and falls
// back to theta = |p_u| without one.  Here r(theta) is cut at its turning points in theta > 0 -- the sign changes of r'(theta), a quartic in theta^2, found ONCE
// when the camera is set (prepare) -- into at most five monotone segments; the smallest root for a radius lies in the first segment whose range holds it and is
// found there by a bracketed Newton iteration with a fixed bound; a radius no segment holds takes the fallback.  Same choice as the reference's (several positive
// roots: the smallest; none: the radius), no eigen-solver per point.  Every loop has a fixed bound, whatever the coordinates (NaN and infinities included).
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/groundfusion_hip.h"   // gf_camera_model, GF_CAMERA_*

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define GF_CAM_HD __host__ __device__ inline
#else
#define GF_CAM_HD inline
#endif

namespace gfcam {

constexpr int kMaxTurn = 4;        // r'(theta) is a quartic in theta^2
constexpr int kNewtonMax = 64;     // steps of the bracketed Newton iteration (each at least halves the bracket or is a Newton step inside it)
constexpr int kGrowMax = 64;       // times the open last segment's far end is multiplied by 4

constexpr int kFullPasses = 9;     // PinholeFullCamera.cc:565-570: j = 0 .. max_cnt = 8
constexpr int kScaPoly = 5, kScaInvPoly = 20;   // SCARAMUZZA_POLY_SIZE, SCARAMUZZA_INV_POLY_SIZE (ScaramuzzaCamera.h)

// A gf_camera_model or gf_camera_model_ex as lift and projection read it: checked (prepare), with the turning points of the Kannala-Brandt r(theta).
struct Camera {
    int32_t model, n_turn;
    double proj[4], dist[8], xi;                     // dist[4 .. 7]: PINHOLE_FULL's k3 k4 k5 k6
    double theta_turn[kMaxTurn], r_turn[kMaxTurn];   // ascending theta; r by kb_r_horner
    double sca[11];                                  // SCARAMUZZA, what its lift reads: poly p0..p4, ac ad ae cx cy, 1 / (ac - ad ae)
    double inv_poly[kScaInvPoly];                    // SCARAMUZZA, read by the projection alone (host)
};

// ---- the radial-tangential distortion PINHOLE and MEI share (PinholeCamera.cc:646-662, CataCamera.cc:766-782)
GF_CAM_HD void distortion(double k1, double k2, double p1, double p2, double x, double y, double& dx, double& dy) {
    double mx2 = x * x, my2 = y * y, mxy = x * y, rho2 = mx2 + my2, rad = k1 * rho2 + k2 * rho2 * rho2;
    dx = x * rad + 2.0 * p1 * mxy + p2 * (rho2 + 2.0 * mx2);
    dy = y * rad + 2.0 * p2 * mxy + p1 * (rho2 + 2.0 * my2);
}
GF_CAM_HD bool no_distortion(double k1, double k2, double p1, double p2) { return k1 == 0.0 && k2 == 0.0 && p1 == 0.0 && p2 == 0.0; }
// pixel -> the undistorted point of the normalised plane: m_inv_K, then eight fixed-point steps of `distortion` (PinholeCamera.cc:450-510, CataCamera.cc:556-612)
GF_CAM_HD void undistort(double fx, double fy, double cx, double cy, double k1, double k2, double p1, double p2, double u, double v, double& X, double& Y) {
    const double i11 = 1.0 / fx, i13 = -cx / fx, i22 = 1.0 / fy, i23 = -cy / fy;
    const double mx_d = i11 * u + i13, my_d = i22 * v + i23;
    if (no_distortion(k1, k2, p1, p2)) { X = mx_d; Y = my_d; return; }
    double dux, duy;
    distortion(k1, k2, p1, p2, mx_d, my_d, dux, duy);
    double mx_u = mx_d - dux, my_u = my_d - duy;
    for (int i = 1; i < 8; ++i) { distortion(k1, k2, p1, p2, mx_u, my_u, dux, duy); mx_u = mx_d - dux; my_u = my_d - duy; }
    X = mx_u; Y = my_u;
}
// the normalised point -> pixel (PinholeCamera.cc:520-542; the tail of CataCamera.cc:636-659)
GF_CAM_HD void distort_to_plane(double fx, double fy, double cx, double cy, double k1, double k2, double p1, double p2, double xu, double yu, double& u, double& v) {
    double xd = xu, yd = yu;
    if (!no_distortion(k1, k2, p1, p2)) { double dx, dy; distortion(k1, k2, p1, p2, xu, yu, dx, dy); xd = xu + dx; yd = yu + dy; }
    u = fx * xd + cx; v = fy * yd + cy;
}

// ---- Kannala-Brandt
// r(theta) as EquidistantCamera.h:160-168 writes it: what spaceToPlane evaluates
GF_CAM_HD double kb_r(double k2, double k3, double k4, double k5, double t) {
    return t + k2 * t * t * t + k3 * t * t * t * t * t + k4 * t * t * t * t * t * t * t + k5 * t * t * t * t * t * t * t * t * t;
}
// the same polynomial and its derivative by Horner in theta^2: what the root search and the turning table evaluate
GF_CAM_HD double kb_r_horner(const double* k, double t) { const double s = t * t; return t * (1.0 + s * (k[0] + s * (k[1] + s * (k[2] + s * k[3])))); }
GF_CAM_HD double kb_dr_horner(const double* k, double t) { const double s = t * t; return 1.0 + s * (3.0 * k[0] + s * (5.0 * k[1] + s * (7.0 * k[2] + s * (9.0 * k[3])))); }

// The root of r(theta) = rho in [a, b], on which r is monotone with rho between r(a) and r(b): Newton steps kept inside a shrinking bracket, a bisection
// where one leaves it or the slope vanishes.  At most kNewtonMax evaluations on any input.
GF_CAM_HD double kb_solve(const double* k, double rho, double a, double ra, double b, double rb) {
    if (ra == rho) return a;
    if (rb == rho) return b;
    double lo = a, hi = b;            // r(lo) < rho < r(hi)
    if (ra > rb) { lo = b; hi = a; }
    double x = (rho > a && rho < b) ? rho : 0.5 * (lo + hi);   // r(theta) = theta + ..: the radius itself is the natural start
    for (int it = 0; it < kNewtonMax; it++) {
        const double f = kb_r_horner(k, x) - rho, d = kb_dr_horner(k, x);
        if (f == 0.0) return x;
        if (f < 0.0) lo = x; else hi = x;
        double xn = x - f / d;
        const double l = lo < hi ? lo : hi, h = lo < hi ? hi : lo;
        if (!(xn > l && xn < h)) xn = 0.5 * (lo + hi);   // also a NaN step
        const double dx = fabs(xn - x);
        x = xn;
        if (dx <= 4.0 * 2.220446049250313e-16 * fabs(x)) break;
    }
    return x;
}

// theta of backprojectSymmetric for |p_u| = rho (EquidistantCamera.cc:731-817): the smallest non-negative real root of r(theta) = rho, rho itself without one
GF_CAM_HD double kb_theta(const Camera& c, double rho) {
    const double* k = c.dist;
    if (k[0] == 0.0 && k[1] == 0.0 && k[2] == 0.0 && k[3] == 0.0) return rho;   // npow == 1
    double a = 0.0, ra = 0.0;
    const int nt = c.n_turn;
    for (int i = 0; i < nt; i++) {
        const double b = c.theta_turn[i], rb = c.r_turn[i];
        if ((ra <= rho && rho <= rb) || (rb <= rho && rho <= ra)) return kb_solve(k, rho, a, ra, b, rb);
        a = b; ra = rb;
    }
    // the open last segment: r runs to +inf or -inf with the sign of the leading coefficient (prepare: the non-zero ones are a prefix)
    const double lead = k[3] != 0.0 ? k[3] : k[2] != 0.0 ? k[2] : k[1] != 0.0 ? k[1] : k[0];
    const bool up = lead > 0.0;
    if (!(up ? ra <= rho : rho <= ra)) return rho;   // no root (and NaN)
    double b = a > 1.0 ? a : 1.0, rb = ra;
    bool found = false;
    for (int g = 0; g < kGrowMax; g++) {
        b *= 4.0;
        rb = kb_r_horner(k, b);
        if (up ? rb >= rho : rb <= rho) { found = true; break; }
    }
    if (!found) return rho;   // a radius beyond every finite bracket: out of any image
    return kb_solve(k, rho, a, ra, b, rb);
}

// ---- PINHOLE_FULL: OpenCV's rational model, k1 k2 p1 p2 k3 k4 k5 k6 in dist[0 .. 7]
// PinholeFullCamera.cc:535-607.  The reference's loop ends on `j > max_cnt` alone: `int min_error = 0.01` is 0, `error` is computed from xd, yd that are never
// assigned, and no distance is < 0.  The definition here is its nine passes (j = 0 .. 8) without the error test and without the unused re-projection
// (:583-603): the ninth iterate, not the true inverse.
GF_CAM_HD void full_lift(const Camera& c, double u, double v, double* P) {
    const double fx = c.proj[0], fy = c.proj[1], cx = c.proj[2], cy = c.proj[3];
    const double k1 = c.dist[0], k2 = c.dist[1], p1 = c.dist[2], p2 = c.dist[3], k3 = c.dist[4], k4 = c.dist[5], k5 = c.dist[6], k6 = c.dist[7];
    const double ifx = 1. / fx, ify = 1. / fy, i13 = -cx / fx, i23 = -cy / fy;   // :548-549, m_inv_K13, m_inv_K23 :375-377
    const double mx_d = ifx * u + i13, my_d = ify * v + i23;                     // :554-555
    double x = mx_d, y = my_d;
    const double x0 = x, y0 = y;
    for (int j = 0; j < kFullPasses; j++) {
        const double r2 = x * x + y * y;                                                                             // :574
        const double icdist = (1 + ((k6 * r2 + k5) * r2 + k4) * r2) / (1 + ((k3 * r2 + k2) * r2 + k1) * r2);         // :575-576
        const double deltaX = 2 * p1 * x * y + p2 * (r2 + 2 * x * x);                                                // :577
        const double deltaY = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y;                                                // :578
        x = (x0 - deltaX) * icdist;                                                                                  // :580
        y = (y0 - deltaY) * icdist;                                                                                  // :581
    }
    P[0] = x; P[1] = y; P[2] = 1.0;                                                                                  // :606
}
// The tail of PinholeFullCamera::spaceToPlane behind p_u (:630-644) with distortion (:754-780): p_d = p_u + d_u, d_u written with its `- x`.  m_noDistortion
// (:630-633) gives the same value, so there is no branch.  Also what the depth registration projects through (gf_depth_reg.hpp).
GF_CAM_HD void full_distort_to_plane(double fx, double fy, double cx, double cy, double k1, double k2, double p1, double p2, double k3, double k4, double k5, double k6,
                                     double x, double y, double& u, double& v) {
    const double r2 = x * x + y * y, r4 = r2 * r2, r6 = r4 * r2;                 // :770-772
    const double a1 = 2 * x * y, a2 = r2 + 2 * x * x, a3 = r2 + 2 * y * y;       // :773-775
    const double cdist = 1 + k1 * r2 + k2 * r4 + k3 * r6;                        // :776
    const double icdist2 = 1. / (1 + k4 * r2 + k5 * r4 + k6 * r6);               // :777
    const double dux = x * cdist * icdist2 + p1 * a1 + p2 * a2 - x;              // :779
    const double duy = y * cdist * icdist2 + p1 * a3 + p2 * a1 - y;              // :780
    u = fx * (x + dux) + cx; v = fy * (y + duy) + cy;                            // :639, :643-644
}

// ---- SCARAMUZZA (OCamCalib).  sca: poly p0..p4, ac ad ae cx cy, m_inv_scale = 1 / (ac - ad ae) (ScaramuzzaCamera.cc:200)
// ScaramuzzaCamera.cc:599-622, with its quirk: phi is the norm of the affine-corrected xc_a, the ray is built from the UNCORRECTED xc.
GF_CAM_HD void scaramuzza_lift(const Camera& c, double u, double v, double* P) {
    const double* s = c.sca;
    const double ac = s[5], ad = s[6], ae = s[7], inv_scale = s[10];
    const double xc0 = u - s[8], xc1 = v - s[9];                                              // :602
    const double xa0 = inv_scale * (xc0 - ad * xc1), xa1 = inv_scale * (-ae * xc0 + ac * xc1);   // :606-609
    const double phi = sqrt(xa0 * xa0 + xa1 * xa1);                                           // :611
    double phi_i = 1.0, z = 0.0;
    for (int i = 0; i < kScaPoly; i++) { z += phi_i * s[i]; phi_i *= phi; }                   // :615-619
    P[0] = xc0; P[1] = xc1; P[2] = -z;                                                        // :621
}
// ScaramuzzaCamera.cc:632-655.  A ray on the axis has norm == 0: invNorm is infinite and 0 * inf makes the pixel non-finite, as in the reference.
GF_CAM_HD void scaramuzza_to_plane(const Camera& c, const double* P, double& u, double& v) {
    const double* s = c.sca;
    const double norm = sqrt(P[0] * P[0] + P[1] * P[1]);                                      // :634
    const double theta = atan2(-P[2], norm);                                                  // :635
    double rho = 0.0, theta_i = 1.0;
    for (int i = 0; i < kScaInvPoly; i++) { rho += theta_i * c.inv_poly[i]; theta_i *= theta; }   // :639-643
    const double invNorm = 1.0 / norm;                                                        // :645
    const double xn0 = P[0] * invNorm * rho, xn1 = P[1] * invNorm * rho;                      // :646-649
    u = xn0 * s[5] + xn1 * s[6] + s[8];                                                       // :651
    v = xn0 * s[7] + xn1 + s[9];                                                              // :652
}

// ---- the five models.  P: the ray liftProjective returns; the caller's float pair is (float)(P[0] / P[2]), (float)(P[1] / P[2]) (feature_tracker.cpp:803-805)
GF_CAM_HD void lift(const Camera& c, double u, double v, double* P) {
    if (c.model == GF_CAMERA_KANNALA_BRANDT) {
        const double i11 = 1.0 / c.proj[0], i13 = -c.proj[2] / c.proj[0], i22 = 1.0 / c.proj[1], i23 = -c.proj[3] / c.proj[1];
        const double px = i11 * u + i13, py = i22 * v + i23;
        const double rho = sqrt(px * px + py * py);
        const double phi = rho < 1e-10 ? 0.0 : atan2(py, px);
        const double theta = kb_theta(c, rho);
        const double st = sin(theta);
        P[0] = st * cos(phi); P[1] = st * sin(phi); P[2] = cos(theta);
        return;
    }
    if (c.model == GF_CAMERA_PINHOLE_FULL) { full_lift(c, u, v, P); return; }
    if (c.model == GF_CAMERA_SCARAMUZZA) { scaramuzza_lift(c, u, v, P); return; }
    double mx, my;
    undistort(c.proj[0], c.proj[1], c.proj[2], c.proj[3], c.dist[0], c.dist[1], c.dist[2], c.dist[3], u, v, mx, my);
    P[0] = mx; P[1] = my;
    if (c.model == GF_CAMERA_PINHOLE) { P[2] = 1.0; return; }
    const double xi = c.xi;
    if (xi == 1.0) P[2] = (1.0 - mx * mx - my * my) / 2.0;
    else { const double rho2 = mx * mx + my * my; P[2] = 1.0 - xi * (rho2 + 1.0) / (xi + sqrt(1.0 + (1.0 - xi * xi) * rho2)); }
}
GF_CAM_HD void lift_pair(const Camera& c, double u, double v, double* P, float& x, float& y) {
    lift(c, u, v, P);
    x = (float)(P[0] / P[2]); y = (float)(P[1] / P[2]);
}

GF_CAM_HD void space_to_plane(const Camera& c, const double* P, double& u, double& v) {
    if (c.model == GF_CAMERA_KANNALA_BRANDT) {
        const double theta = acos(P[2] / sqrt(P[0] * P[0] + P[1] * P[1] + P[2] * P[2])), phi = atan2(P[1], P[0]);
        const double r = kb_r(c.dist[0], c.dist[1], c.dist[2], c.dist[3], theta);
        u = c.proj[0] * (r * cos(phi)) + c.proj[2]; v = c.proj[1] * (r * sin(phi)) + c.proj[3];
        return;
    }
    if (c.model == GF_CAMERA_PINHOLE_FULL) {   // p_u, :628
        const double* d = c.dist;
        full_distort_to_plane(c.proj[0], c.proj[1], c.proj[2], c.proj[3], d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7], P[0] / P[2], P[1] / P[2], u, v);
        return;
    }
    if (c.model == GF_CAMERA_SCARAMUZZA) { scaramuzza_to_plane(c, P, u, v); return; }
    const double z = c.model == GF_CAMERA_MEI ? P[2] + c.xi * sqrt(P[0] * P[0] + P[1] * P[1] + P[2] * P[2]) : P[2];
    distort_to_plane(c.proj[0], c.proj[1], c.proj[2], c.proj[3], c.dist[0], c.dist[1], c.dist[2], c.dist[3], P[0] / z, P[1] / z, u, v);
}

// ---- what camera_lift_kernel (gf_camera_kernels.hpp) is launched with, for the translation units that launch it without holding it
struct alignas(8) Pair { float x, y; };   // a float pair as it lies in the tables (the device side's float2)
constexpr int kLiftSets = 3;              // the tracker lifts up to three tables per call: LK's points, the new corners, and the right points of its stereo sequences
// One table of points per list entry.  With LiftArgs::first the points of entry b are pts[first[b] .. first[b + 1]) (n is not read); without, row b of `cap`
// points of which n[b] are lifted (n == nullptr: none).
// cams / cam_of: the set's own cameras and list (the right cameras of the stereo branch), or null: LiftArgs's
struct LiftSet { const Pair* pts; const int* n; Pair* un; double* rays; const struct Camera* cams = nullptr; const int* cam_of = nullptr; };   // rays: 3 doubles per point, or null
struct LiftArgs {
    const Camera* cams;    // the checked cameras (gfcam::prepare)
    const int* cam_of;     // [batch] which camera entry b has, < 0: the entry is skipped; null: cams[b]
    const int* first;      // [batch + 1] offsets, or null: rows of `cap`
    int cap, batch, n_sets;
    LiftSet set[kLiftSets];
};

// ---- host side: what a setter checks, and the turning table

inline const char* model_name(int m) {
    return m == GF_CAMERA_PINHOLE ? "PINHOLE" : m == GF_CAMERA_MEI ? "MEI" : m == GF_CAMERA_KANNALA_BRANDT ? "KANNALA_BRANDT" : m == GF_CAMERA_PINHOLE_FULL ? "PINHOLE_FULL" :
           m == GF_CAMERA_SCARAMUZZA ? "SCARAMUZZA" : "?";
}
inline const char* proj_name(int m, int i) {
    static const char* const n[4][4] = {{"fx", "fy", "cx", "cy"}, {"gamma1", "gamma2", "u0", "v0"}, {"mu", "mv", "u0", "v0"}, {"fx", "fy", "cx", "cy"}};
    return n[m][i];
}
inline const char* dist_name(int m, int i) {
    static const char* const n[3][4] = {{"k1", "k2", "p1", "p2"}, {"k1", "k2", "p1", "p2"}, {"k2", "k3", "k4", "k5"}};
    return n[m][i];
}

// The sign changes of p(s) = a[0] + a[1] s + .. + a[deg] s^deg in s > 0, ascending, at most deg of them: between two neighbouring sign changes of p' (found the
// same way, one degree down) p is monotone, so a bisection per interval finds each.  A root where p touches zero without crossing is no sign change and is not
// reported: r keeps its direction there.
inline int sign_changes(const double* a, int deg, double* out) {
    while (deg > 0 && a[deg] == 0.0) deg--;
    if (deg <= 0) return 0;
    double bound = 0.0;   // Cauchy: every root lies below 1 + max |a_i / a_deg|
    for (int i = 0; i < deg; i++) { const double q = fabs(a[i] / a[deg]); if (q > bound) bound = q; }
    bound += 1.0;
    double d[kMaxTurn + 1], cut[kMaxTurn + 2];
    for (int i = 1; i <= deg; i++) d[i - 1] = a[i] * i;
    int nc = sign_changes(d, deg - 1, cut + 1);
    cut[0] = 0.0;
    while (nc > 0 && cut[nc] >= bound) nc--;
    cut[nc + 1] = bound;
    auto p = [&](double s) { double v = a[deg]; for (int i = deg - 1; i >= 0; i--) v = v * s + a[i]; return v; };
    int n = 0;
    for (int i = 0; i <= nc; i++) {
        double lo = cut[i], hi = cut[i + 1];
        const bool plo = p(lo) > 0.0, phi = p(hi) > 0.0;
        if (plo == phi) continue;
        for (int it = 0; it < 200; it++) {
            const double mid = 0.5 * (lo + hi);
            if (!(mid > lo && mid < hi)) break;
            if ((p(mid) > 0.0) == plo) lo = mid; else hi = mid;
        }
        if (hi > 0.0) out[n++] = hi;
    }
    return n;
}

// Checks `m` and fills `c`.  False with a message that names the field: a model that is none of the three, reserved != 0, a value that is not finite, a focal
// parameter <= 0, xi < 0, and a Kannala-Brandt set in which a zero coefficient precedes a non-zero one (EquidistantCamera.cc:731-782 counts the zero
// coefficients instead of locating them and divides the companion column by coeffs(npow), which for such a set is one of the zeros: the reference divides by
// zero, there is nothing to be faithful to).
inline bool prepare(const gf_camera_model& m, Camera& c, char* msg, size_t n) {
    if (m.model != GF_CAMERA_PINHOLE && m.model != GF_CAMERA_MEI && m.model != GF_CAMERA_KANNALA_BRANDT) {
        snprintf(msg, n, "gf_camera_model.model %d is none of GF_CAMERA_PINHOLE, GF_CAMERA_MEI, GF_CAMERA_KANNALA_BRANDT", m.model); return false;
    }
    if (m.reserved != 0) { snprintf(msg, n, "gf_camera_model.reserved must be 0, got %d", m.reserved); return false; }
    for (int i = 0; i < 4; i++) if (!isfinite(m.proj[i])) { snprintf(msg, n, "gf_camera_model.proj[%d] (%s %s) is not finite", i, model_name(m.model), proj_name(m.model, i)); return false; }
    for (int i = 0; i < 4; i++) if (!isfinite(m.dist[i])) { snprintf(msg, n, "gf_camera_model.dist[%d] (%s %s) is not finite", i, model_name(m.model), dist_name(m.model, i)); return false; }
    for (int i = 0; i < 2; i++) if (!(m.proj[i] > 0.0)) { snprintf(msg, n, "gf_camera_model.proj[%d] (%s %s) must be > 0, got %g", i, model_name(m.model), proj_name(m.model, i), m.proj[i]); return false; }
    if (m.model == GF_CAMERA_MEI) {
        if (!isfinite(m.xi)) { snprintf(msg, n, "gf_camera_model.xi is not finite"); return false; }
        if (m.xi < 0.0) { snprintf(msg, n, "gf_camera_model.xi must be >= 0, got %g", m.xi); return false; }
    }
    if (m.model == GF_CAMERA_KANNALA_BRANDT)
        for (int i = 0; i < 3; i++)
            for (int j = i + 1; j < 4; j++)
                if (m.dist[i] == 0.0 && m.dist[j] != 0.0) {
                    snprintf(msg, n, "gf_camera_model.dist[%d] (KANNALA_BRANDT %s) is zero while dist[%d] (%s) is not: the reference's backprojectSymmetric divides by zero for such a set",
                             i, dist_name(m.model, i), j, dist_name(m.model, j));
                    return false;
                }
    c = Camera{};
    c.model = m.model;
    for (int i = 0; i < 4; i++) { c.proj[i] = m.proj[i]; c.dist[i] = m.dist[i]; }
    c.xi = m.model == GF_CAMERA_MEI ? m.xi : 0.0;
    if (m.model == GF_CAMERA_KANNALA_BRANDT) {
        const double q[5] = {1.0, 3.0 * m.dist[0], 5.0 * m.dist[1], 7.0 * m.dist[2], 9.0 * m.dist[3]};   // r'(theta) in s = theta^2
        double s[kMaxTurn];
        c.n_turn = sign_changes(q, 4, s);
        for (int i = 0; i < c.n_turn; i++) { c.theta_turn[i] = sqrt(s[i]); c.r_turn[i] = kb_r_horner(c.dist, c.theta_turn[i]); }
    }
    return true;
}

// The same for the wide struct, which holds all five models.  Models 0-2: the 80-byte checker on the fields gf_camera_model has (the rest is not read).
// PINHOLE_FULL: fx, fy > 0.  SCARAMUZZA: proj and dist are not read; ac - ad ae == 0 is refused, the reference divides by it (ScaramuzzaCamera.cc:200).
inline gf_camera_model narrow(const gf_camera_model_ex& w) {   // the fields gf_camera_model has; meaningful for models 0-2
    gf_camera_model m{};
    m.model = w.model; m.reserved = w.reserved;
    for (int i = 0; i < 4; i++) { m.proj[i] = w.proj[i]; m.dist[i] = w.dist[i]; }
    m.xi = w.xi;
    return m;
}
inline gf_camera_model_ex widen(const gf_camera_model& m) {
    gf_camera_model_ex w{};
    w.model = m.model; w.reserved = m.reserved;
    for (int i = 0; i < 4; i++) { w.proj[i] = m.proj[i]; w.dist[i] = m.dist[i]; }
    w.xi = m.xi;
    return w;
}
inline bool prepare(const gf_camera_model_ex& m, Camera& c, char* msg, size_t n) {
    if (m.model < GF_CAMERA_PINHOLE || m.model > GF_CAMERA_SCARAMUZZA) {
        snprintf(msg, n, "gf_camera_model_ex.model %d is none of GF_CAMERA_PINHOLE, GF_CAMERA_MEI, GF_CAMERA_KANNALA_BRANDT, GF_CAMERA_PINHOLE_FULL, GF_CAMERA_SCARAMUZZA", m.model);
        return false;
    }
    if (m.reserved != 0) { snprintf(msg, n, "gf_camera_model_ex.reserved must be 0, got %d", m.reserved); return false; }
    if (m.model <= GF_CAMERA_KANNALA_BRANDT) return prepare(narrow(m), c, msg, n);
    if (m.model == GF_CAMERA_PINHOLE_FULL) {
        static const char* const dn[8] = {"k1", "k2", "p1", "p2", "k3", "k4", "k5", "k6"};
        for (int i = 0; i < 4; i++) if (!isfinite(m.proj[i])) { snprintf(msg, n, "gf_camera_model_ex.proj[%d] (PINHOLE_FULL %s) is not finite", i, proj_name(m.model, i)); return false; }
        for (int i = 0; i < 8; i++) if (!isfinite(m.dist[i])) { snprintf(msg, n, "gf_camera_model_ex.dist[%d] (PINHOLE_FULL %s) is not finite", i, dn[i]); return false; }
        for (int i = 0; i < 2; i++) if (!(m.proj[i] > 0.0)) { snprintf(msg, n, "gf_camera_model_ex.proj[%d] (PINHOLE_FULL %s) must be > 0, got %g", i, proj_name(m.model, i), m.proj[i]); return false; }
        c = Camera{};
        c.model = m.model;
        for (int i = 0; i < 4; i++) c.proj[i] = m.proj[i];
        for (int i = 0; i < 8; i++) c.dist[i] = m.dist[i];
        return true;
    }
    static const char* const an[5] = {"ac", "ad", "ae", "cx", "cy"};
    for (int i = 0; i < kScaPoly; i++) if (!isfinite(m.poly[i])) { snprintf(msg, n, "gf_camera_model_ex.poly[%d] (SCARAMUZZA poly_parameters p%d) is not finite", i, i); return false; }
    for (int i = 0; i < kScaInvPoly; i++) if (!isfinite(m.inv_poly[i])) { snprintf(msg, n, "gf_camera_model_ex.inv_poly[%d] (SCARAMUZZA inv_poly_parameters p%d) is not finite", i, i); return false; }
    for (int i = 0; i < 5; i++) if (!isfinite(m.affine[i])) { snprintf(msg, n, "gf_camera_model_ex.affine[%d] (SCARAMUZZA %s) is not finite", i, an[i]); return false; }
    const double det = m.affine[0] - m.affine[1] * m.affine[2];
    if (det == 0.0) { snprintf(msg, n, "gf_camera_model_ex.affine: ac - ad * ae is 0 (SCARAMUZZA ac %g, ad %g, ae %g): the reference divides by it", m.affine[0], m.affine[1], m.affine[2]); return false; }
    c = Camera{};
    c.model = m.model;
    for (int i = 0; i < kScaPoly; i++) c.sca[i] = m.poly[i];
    for (int i = 0; i < 5; i++) c.sca[5 + i] = m.affine[i];
    c.sca[10] = 1.0 / det;                                   // m_inv_scale, ScaramuzzaCamera.cc:200
    for (int i = 0; i < kScaInvPoly; i++) c.inv_poly[i] = m.inv_poly[i];
    return true;
}

// the pinhole of a sequence's gf_tracker_seq_cfg: what a sequence runs with ahead of any camera setter
inline gf_camera_model pinhole_of(const gf_tracker_seq_cfg& s) {
    gf_camera_model m{};
    m.model = GF_CAMERA_PINHOLE;
    m.proj[0] = s.fx; m.proj[1] = s.fy; m.proj[2] = s.cx; m.proj[3] = s.cy;
    m.dist[0] = s.k1; m.dist[1] = s.k2; m.dist[2] = s.p1; m.dist[3] = s.p2;
    return m;
}

}  // namespace gfcam
