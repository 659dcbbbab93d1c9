// gf_stereo_depth.hpp — the depth a left-to-right match determines (gf_stereo_depth_cfg; gf_tracker_set_seq_stereo_depth, gf_stereo_depth_batch*): what fills the
// eighth field of a stereo sequence's left observations, where the reference's stereo branch would read the right image as 16-bit millimetres
// (feature_tracker.cpp:344-368).  A definition of this repository ("Stereo depth"): the reference's triangulatePoint goes through a Jacobi SVD,
// which cannot be restated bit for bit, and nothing in the reference calls it on this path.
// Plain C++ in double precision that host and device both compile, one source for the kernel (gf_stereo_depth_kernels.hpp), the tracker's host stage
// (GF_STEREO_DEPTH_HOST=1), the building blocks and the stand-alone host program of the tests (tests/native/stereo_depth_host.cpp).  It sets no floating-point
// contraction of its own; the library compiles it without contraction on both sides, and nothing here but +, -, *, /, rint, fabs and comparisons touches a double
// behind the two lifts, so host and device give the same bits for the models whose lift has no transcendental (every one but KANNALA_BRANDT).
//
// One point: the left pixel (ul, vl) and the right pixel (ur, vr) as the floats the tables hold, the match status, the two checked cameras, and a rig
// p_left = R p_right + t.
//   1. P_l = lift(left, ul, vl), P_r = lift(right, ur, vr) in double (gfcam::lift: the kernel's own lifts, not the float pairs of the observations).
//   2. a = (P_l.x / P_l.z, P_l.y / P_l.z, 1), b = (P_r.x / P_r.z, P_r.y / P_r.z, 1), d = R b, each row summed as (R0 b.x + R1 b.y) + R2.
//   3. min |s a - t - u d|^2 in closed form.  dot(x, y) = (x0 y0 + x1 y1) + x2 y2; aa = a.a, dd = d.d, ad = a.d, at = a.t, dt = d.t, den = aa dd - ad ad,
//      s = (at dd - ad dt) / den, u = (at ad - aa dt) / den.
//   4. s is the depth along the left camera's z axis (a.z == 1): what triangulateWithDepth multiplies `point` by.
// The gates, in this order; the first that fires names the reason, and every reason but kOk yields 0:
//   kNoMatch   status == 0
//   kLift      a ray component that is not finite, P_l.z <= 0 or P_r.z <= 0
//   kParallax  den <= (min_parallax^2 aa) dd                      (den / (aa dd) is the squared sine of the angle between the rays)
//   kBehind    s <= 0 or u <= 0
//   kEpipolar  q = R^T (s a - t), each component summed as (R[j] w0 + R[3 + j] w1) + R[6 + j] w2:  q.z <= 0, or
//              (q.x - b.x q.z)^2 + (q.y - b.y q.z)^2 > max_epipolar^2 (q.z q.z)                     (no division)
//   kRange     m = rint(1000 s), round half to even: not (lo <= m <= hi), lo = 1000 min_depth, hi = min(1000 max_depth, 65535).  A NaN that the steps above let
//              through ends here.
//   kOk        depth = (uint16_t)m
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/groundfusion_hip.h"   // gf_stereo_depth_cfg
#include "gf_camera_models.hpp"               // gfcam::Camera, gfcam::lift

#if defined(__HIPCC__) || defined(__HIP__)
#define GF_SD_HD __host__ __device__ inline
#else
#define GF_SD_HD inline
#endif

namespace gfsd {

// the reason codes, in the order the gates are tested; 0 is what a byte holds that nothing wrote
enum Why : uint8_t { kUnwritten = 0, kNoMatch = 1, kLift = 2, kParallax = 3, kBehind = 4, kEpipolar = 5, kRange = 6, kOk = 7 };
constexpr int kReasons = 8;

// the defaults of the gates gf_stereo_depth_from_yaml does not find in a config file ("Stereo depth", has the reasoning)
constexpr double kMinParallax = 1e-3;          // sine of the ray angle: under half a pixel of disparity at FOCAL_LENGTH 460, below what LK resolves
constexpr double kMaxEpipolar = 10.0 / 460.0;  // the residual triangulateWithDepth allows (feature_manager.cpp:773), in the right eye's normalised plane
constexpr double kMinDepth = 0.1;              // the estimator skips depths below it
constexpr double kMaxCount = 65535.0;

// A checked gf_stereo_depth_cfg as depth_of reads it
struct Rig { double R[9], t[3], par2, epi2, lo, hi; };

GF_SD_HD bool finite(double v) { return fabs(v) <= 1.7976931348623157e308; }   // false for NaN too
GF_SD_HD double dot3(const double* x, const double* y) { return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]; }

struct Depth { uint16_t mm; uint8_t why; };

GF_SD_HD Depth depth_of(const gfcam::Camera& left, const gfcam::Camera& right, const Rig& g, float ul, float vl, float ur, float vr, uint8_t status) {
    if (!status) return {0, kNoMatch};
    double Pl[3], Pr[3];
    gfcam::lift(left, (double)ul, (double)vl, Pl);
    gfcam::lift(right, (double)ur, (double)vr, Pr);
    if (!finite(Pl[0]) || !finite(Pl[1]) || !finite(Pl[2]) || !finite(Pr[0]) || !finite(Pr[1]) || !finite(Pr[2]) || Pl[2] <= 0.0 || Pr[2] <= 0.0) return {0, kLift};
    const double a[3] = {Pl[0] / Pl[2], Pl[1] / Pl[2], 1.0};
    const double bx = Pr[0] / Pr[2], by = Pr[1] / Pr[2];
    const double d[3] = {(g.R[0] * bx + g.R[1] * by) + g.R[2], (g.R[3] * bx + g.R[4] * by) + g.R[5], (g.R[6] * bx + g.R[7] * by) + g.R[8]};
    const double aa = dot3(a, a), dd = dot3(d, d), ad = dot3(a, d), at = dot3(a, g.t), dt = dot3(d, g.t);
    const double den = aa * dd - ad * ad;
    if (den <= (g.par2 * aa) * dd) return {0, kParallax};
    const double s = (at * dd - ad * dt) / den, u = (at * ad - aa * dt) / den;
    if (s <= 0.0 || u <= 0.0) return {0, kBehind};
    const double w0 = s * a[0] - g.t[0], w1 = s * a[1] - g.t[1], w2 = s * a[2] - g.t[2];
    const double qx = (g.R[0] * w0 + g.R[3] * w1) + g.R[6] * w2, qy = (g.R[1] * w0 + g.R[4] * w1) + g.R[7] * w2, qz = (g.R[2] * w0 + g.R[5] * w1) + g.R[8] * w2;
    if (qz <= 0.0) return {0, kEpipolar};
    const double ex = qx - bx * qz, ey = qy - by * qz;
    if (ex * ex + ey * ey > g.epi2 * (qz * qz)) return {0, kEpipolar};
    const double m = rint(1000.0 * s);
    if (!(m >= g.lo && m <= g.hi)) return {0, kRange};
    return {(uint16_t)m, kOk};
}

// ---- host side: what a setter checks
// False with a message that names the field: enable or right_obs outside {0, 1}, a value that is not finite, an R with |R R^T - I| > 1e-9 in an entry or
// |det R - 1| > 1e-9, t == 0, a gate that is not positive, min_depth >= max_depth, max_depth > 65.535.
inline bool check(const gf_stereo_depth_cfg& c, char* msg, size_t n) {
    if (c.enable != 0 && c.enable != 1) { snprintf(msg, n, "gf_stereo_depth_cfg.enable must be 0 or 1, got %d", c.enable); return false; }
    if (c.right_obs != 0 && c.right_obs != 1) { snprintf(msg, n, "gf_stereo_depth_cfg.right_obs must be 0 or 1, got %d", c.right_obs); return false; }
    for (int i = 0; i < 9; i++) if (!finite(c.R[i])) { snprintf(msg, n, "gf_stereo_depth_cfg.R[%d] is not finite", i); return false; }
    for (int i = 0; i < 3; i++) if (!finite(c.t[i])) { snprintf(msg, n, "gf_stereo_depth_cfg.t[%d] is not finite", i); return false; }
    const double v[4] = {c.min_parallax, c.max_epipolar, c.min_depth, c.max_depth};
    static const char* const name[4] = {"min_parallax", "max_epipolar", "min_depth", "max_depth"};
    for (int i = 0; i < 4; i++) if (!finite(v[i])) { snprintf(msg, n, "gf_stereo_depth_cfg.%s is not finite", name[i]); return false; }
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            const double e = c.R[3 * i] * c.R[3 * j] + c.R[3 * i + 1] * c.R[3 * j + 1] + c.R[3 * i + 2] * c.R[3 * j + 2] - (i == j ? 1.0 : 0.0);
            if (!(fabs(e) <= 1e-9)) { snprintf(msg, n, "gf_stereo_depth_cfg.R is no rotation: (R R^T - I)[%d][%d] is %g, beyond 1e-9", i, j, e); return false; }
        }
    const double det = c.R[0] * (c.R[4] * c.R[8] - c.R[5] * c.R[7]) - c.R[1] * (c.R[3] * c.R[8] - c.R[5] * c.R[6]) + c.R[2] * (c.R[3] * c.R[7] - c.R[4] * c.R[6]);
    if (!(fabs(det - 1.0) <= 1e-9)) { snprintf(msg, n, "gf_stereo_depth_cfg.R is no rotation: its determinant is %g, not +1", det); return false; }
    if (c.t[0] == 0.0 && c.t[1] == 0.0 && c.t[2] == 0.0) { snprintf(msg, n, "gf_stereo_depth_cfg.t is 0: a rig without a baseline determines no depth"); return false; }
    for (int i = 0; i < 4; i++) if (!(v[i] > 0.0)) { snprintf(msg, n, "gf_stereo_depth_cfg.%s must be > 0, got %g", name[i], v[i]); return false; }
    if (!(c.min_depth < c.max_depth)) { snprintf(msg, n, "gf_stereo_depth_cfg.min_depth %g must be below max_depth %g", c.min_depth, c.max_depth); return false; }
    if (c.max_depth > 65.535) { snprintf(msg, n, "gf_stereo_depth_cfg.max_depth %g is beyond 65.535 m, the last count of a 16-bit millimetre depth", c.max_depth); return false; }
    return true;
}

inline Rig rig_of(const gf_stereo_depth_cfg& c) {   // c: checked
    Rig g{};
    for (int i = 0; i < 9; i++) g.R[i] = c.R[i];
    for (int i = 0; i < 3; i++) g.t[i] = c.t[i];
    g.par2 = c.min_parallax * c.min_parallax; g.epi2 = c.max_epipolar * c.max_epipolar;
    g.lo = 1000.0 * c.min_depth;
    g.hi = 1000.0 * c.max_depth < kMaxCount ? 1000.0 * c.max_depth : kMaxCount;
    return g;
}

// ---- what stereo_depth_kernel (gf_stereo_depth_kernels.hpp) is launched with, for the translation units that launch it without holding it
// One entry: a sequence of the tracker, or a set of the building block.  on == 0: the positions that name it leave at once.
struct Entry { gfcam::Camera left, right; Rig rig; int32_t on, pad_; };
static_assert(sizeof(Entry) % 8 == 0, "entries lie back to back and are read as dwords");
// No padding anywhere in an Entry, so two entries are equal exactly when their bytes are: what the tracker's shadow of the device table compares
static_assert(sizeof(gfcam::Camera) == 2 * sizeof(int32_t) + (4 + 8 + 1 + 2 * gfcam::kMaxTurn + 11 + gfcam::kScaInvPoly) * sizeof(double), "gfcam::Camera has no padding");
static_assert(sizeof(Rig) == 16 * sizeof(double) && sizeof(Entry) == 2 * sizeof(gfcam::Camera) + sizeof(Rig) + 2 * sizeof(int32_t), "Rig and Entry have no padding");
// Every table below is device memory.  Position b of `count` names entry entry_of[b] (< 0: it leaves at once; null: entry b).
// The points of position b: with `first`, left_pts / right_pts / status / depth_mm / why [first[b] .. first[b + 1]); without, rows of `cap`, and the left point k
// is gathered as the stereo kernel gathers it (gf_stereo_kernels.hpp): k < n_tracked[b] ? lk_pts[row[k]] : new_pts[k - n_tracked[b]], with the same clamps.
struct Args {
    const Entry* entries; const int* entry_of;
    const int* first;
    int cap, count;
    const gfcam::Pair* left_pts;
    const int* n_tracked; const int* row; const gfcam::Pair* lk_pts; const int* n_new; const gfcam::Pair* new_pts;
    const gfcam::Pair* right_pts; const uint8_t* status;
    uint16_t* depth_mm; uint8_t* why;
};

}  // namespace gfsd
