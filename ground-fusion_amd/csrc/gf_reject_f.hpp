// gf_reject_f.hpp — rejectWithF (feature_tracker.cpp:711-743): the epipolar outlier test between LK and the back end, as THIS repository defines it (DESIGN.md
// section 4, "rejectWithF").  cv::findFundamentalMat(FM_RANSAC) cannot be restated bit for bit (its RNG stream, a seven-point cubic, an SVD, an adaptive
// iteration count), so the definition is written down here: one source that the host (gfrf::reject), the kernel (gf_reject_f_kernels.hpp) and a numpy
// restatement (tests/reject_f_ref.py) give the same bytes for.  Nothing but + - * /, sqrt, comparisons and 32-bit integer arithmetic; the translation units
// that include it build with -ffp-contract=off.
//
//   candidates   the rows whose status is 1 and whose four virtual-pixel coordinates are finite, in row order; m of them.  A row with status 1 and a non-finite
//                coordinate gets status 0 whatever m is.  m < 8: nothing else happens (:713).
//   hypotheses   h = 0 .. 511.  Each draws 8 distinct candidates: draw d = 0, 1, .. gives index draw_word(seed, h, d) % m, taken if no earlier taken draw of
//                the hypothesis gave it; void if 8 are not found within kMaxDraws draws.
//   model        Hartley normalisation of the 8 points of each side (void unless both mean distances are > 0), the 8 x 9 system of b^T F a = 0, its null vector
//                by Gaussian elimination with full pivoting (no row or column is moved: a pivot is the largest magnitude among the rows and columns not yet
//                used, ties to the smaller row, then the smaller column; void if it is below kPivotMin), back-substitution with the column left over set to 1,
//                F = Tb^T F Ta.  Rank 2 is not enforced.
//   score        a candidate is an inlier iff r^2 <= t^2 (l2.x^2 + l2.y^2) and r^2 <= t^2 (l1.x^2 + l1.y^2), l2 = F a, l1 = F^T b, r = b . l2.
//   result       the hypothesis with the most inliers, ties to the smaller h; a hypothesis with fewer than 8 inliers (it does not fit its own sample: overflow,
//                NaN) counts as void.  The winner's outliers get status 0.  No hypothesis left: nothing is rejected.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define GF_RF_HD __host__ __device__ inline
#else
#define GF_RF_HD inline
#endif

#ifndef GF_REJECT_F_HYPOTHESES
#define GF_REJECT_F_HYPOTHESES 512   // at 55 % inliers 1 - (1 - 0.55^8)^512 = 0.987: the reference's 0.99 confidence, rounded
#endif

namespace gfrf {

constexpr int kHypotheses = GF_REJECT_F_HYPOTHESES;
constexpr int kSample = 8;
constexpr int kMaxDraws = 64;          // draws of one hypothesis; at m = 8 the expected number for 8 distinct indices is 21.7
constexpr int kMaxCandidates = 1024;   // rows of one set: what the kernel keeps in LDS (16 bytes each)
constexpr double kPivotMin = 1e-12;    // on the normalised system, whose entries are of order 1
constexpr double kFocal = 460.0;       // FOCAL_LENGTH, parameters.h:23
constexpr double kSqrt2 = 1.4142135623730951;   // the double nearest sqrt(2)

struct Cand { float ax, ay, bx, by; };   // a: the previous frame's virtual pixel, b: the current frame's
// what one set's run leaves beside the status bytes
struct Result { int32_t m, rejected, winner, inliers; };   // winner: the hypothesis, -1: none (m < 8 or every hypothesis void); rejected counts the non-finite rows too

// lowbias32 (C. Wellons, public domain): a bijective mix of 32 bits
GF_RF_HD uint32_t mix32(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
    return x;
}
// the seed of a sequence's frame: the setter's seed and the number of frames the sequence has taken (this one included)
GF_RF_HD uint32_t frame_seed(uint32_t seed, uint32_t frames) { return mix32(seed ^ mix32(frames + 0x9e3779b9U)); }
// draw d of hypothesis h: depends on (seed, h, d) alone
GF_RF_HD uint32_t draw_word(uint32_t seed, uint32_t h, uint32_t d) { return mix32(seed ^ mix32(h * (uint32_t)kMaxDraws + d + 1U)); }

// FOCAL_LENGTH * X / Z + width / 2.0 as a cv::Point2f (:722-729)
GF_RF_HD float virtual_pixel(double focal, double X, double Z, int extent) { return (float)(focal * X / Z + (double)extent / 2.0); }

GF_RF_HD bool finite_f(float v) { return v - v == 0.0f; }
GF_RF_HD bool finite_cand(const Cand& c) { return finite_f(c.ax) && finite_f(c.ay) && finite_f(c.bx) && finite_f(c.by); }
GF_RF_HD double abs_d(double v) { return v < 0.0 ? -v : v; }

// The 8 indices of hypothesis h into idx; false: void.
GF_RF_HD bool draw_sample(uint32_t seed, int h, int m, int* idx) {
    int got = 0;
    for (int d = 0; d < kMaxDraws && got < kSample; d++) {
        const int i = (int)(draw_word(seed, (uint32_t)h, (uint32_t)d) % (uint32_t)m);
        bool dup = false;
        for (int k = 0; k < got; k++) dup = dup || idx[k] == i;
        if (!dup) idx[got++] = i;
    }
    return got == kSample;
}

// Hartley's normalisation of one side's 8 points (px, py): centroid c, scale s = sqrt(2) / mean distance.  False: the mean distance is not > 0.
GF_RF_HD bool hartley(const double* px, const double* py, double& cx, double& cy, double& s) {
    double sx = 0.0, sy = 0.0;
    for (int k = 0; k < kSample; k++) { sx = sx + px[k]; sy = sy + py[k]; }
    cx = sx / 8.0; cy = sy / 8.0;
    double sd = 0.0;
    for (int k = 0; k < kSample; k++) { const double dx = px[k] - cx, dy = py[k] - cy; sd = sd + sqrt(dx * dx + dy * dy); }
    const double d = sd / 8.0;
    if (!(d > 0.0)) return false;
    s = kSqrt2 / d;
    return true;
}

// row k of the system for the normalised pair (ax, ay), (bx, by): b^T F a = 0 in F's row-major unknowns
GF_RF_HD void system_row(double ax, double ay, double bx, double by, double* r) {
    r[0] = bx * ax; r[1] = bx * ay; r[2] = bx; r[3] = by * ax; r[4] = by * ay; r[5] = by; r[6] = ax; r[7] = ay; r[8] = 1.0;
}

// One lane's share of an elimination step: the largest magnitude of row `r` over the columns not in col_used, ties to the smaller column.
GF_RF_HD void row_best(const double* r, uint32_t col_used, double& best, int& col) {
    best = -1.0; col = 0;
    for (int c = 0; c < 9; c++) if (!((col_used >> c) & 1U)) { const double v = abs_d(r[c]); if (v > best) { best = v; col = c; } }
}
// row r -= (r[pc] / p[pc]) p over the columns not used
GF_RF_HD void row_eliminate(double* r, const double* p, int pc, uint32_t col_used_after) {
    const double f = r[pc] / p[pc];
    for (int c = 0; c < 9; c++) if (!((col_used_after >> c) & 1U)) r[c] = r[c] - f * p[c];
}
// x from the eliminated system: prow / pcol hold step i's pivot in bits [4 i, 4 i + 4); the column in no step is 1
GF_RF_HD void back_substitute(const double* A, uint32_t prow, uint32_t pcol, uint32_t col_used, double* x) {
    uint32_t solved = ~col_used & 0x1ffU;   // the one column left over
    for (int c = 0; c < 9; c++) x[c] = 1.0;
    for (int i = kSample - 1; i >= 0; i--) {
        const int r = (int)((prow >> (4 * i)) & 15U), pc = (int)((pcol >> (4 * i)) & 15U);
        double acc = 0.0;
        for (int c = 0; c < 9; c++) if ((solved >> c) & 1U) acc = acc + A[9 * r + c] * x[c];
        x[pc] = -acc / A[9 * r + pc];
        solved |= 1U << pc;
    }
}
// F = Tb^T Fn Ta, T = [s 0 -s c.x; 0 s -s c.y; 0 0 1]
GF_RF_HD void denormalise(const double* f, double cax, double cay, double sa, double cbx, double cby, double sb, double* F) {
    double G[9];
    for (int r = 0; r < 3; r++) {
        G[3 * r] = f[3 * r] * sa; G[3 * r + 1] = f[3 * r + 1] * sa;
        G[3 * r + 2] = f[3 * r + 2] - (G[3 * r] * cax + G[3 * r + 1] * cay);
    }
    for (int c = 0; c < 3; c++) {
        F[c] = sb * G[c]; F[3 + c] = sb * G[3 + c];
        F[6 + c] = G[6 + c] - (F[c] * cbx + F[3 + c] * cby);
    }
}
GF_RF_HD bool inlier(const double* F, const Cand& p, double tt) {
    const double ax = (double)p.ax, ay = (double)p.ay, bx = (double)p.bx, by = (double)p.by;
    const double l2x = F[0] * ax + F[1] * ay + F[2], l2y = F[3] * ax + F[4] * ay + F[5], l2z = F[6] * ax + F[7] * ay + F[8];
    const double r = bx * l2x + by * l2y + l2z, rr = r * r;
    const double l1x = F[0] * bx + F[3] * by + F[6], l1y = F[1] * bx + F[4] * by + F[7];
    return rr <= tt * (l2x * l2x + l2y * l2y) && rr <= tt * (l1x * l1x + l1y * l1y);
}

// The model of hypothesis h over the m candidates; false: void.  The serial form (host); the kernel spreads the same steps over 8 lanes.
inline bool model(const Cand* cand, int m, uint32_t seed, int h, double* F) {
    int idx[kSample];
    if (!draw_sample(seed, h, m, idx)) return false;
    double ax[kSample], ay[kSample], bx[kSample], by[kSample];
    for (int k = 0; k < kSample; k++) { const Cand& c = cand[idx[k]]; ax[k] = (double)c.ax; ay[k] = (double)c.ay; bx[k] = (double)c.bx; by[k] = (double)c.by; }
    double cax, cay, sa, cbx, cby, sb;
    if (!hartley(ax, ay, cax, cay, sa) || !hartley(bx, by, cbx, cby, sb)) return false;
    double A[kSample * 9];
    for (int k = 0; k < kSample; k++) system_row((ax[k] - cax) * sa, (ay[k] - cay) * sa, (bx[k] - cbx) * sb, (by[k] - cby) * sb, A + 9 * k);
    uint32_t row_used = 0, col_used = 0, prow = 0, pcol = 0;
    for (int i = 0; i < kSample; i++) {
        double best = -1.0; int pr = 0, pc = 0;
        for (int r = 0; r < kSample; r++) if (!((row_used >> r) & 1U)) {
            double v; int c;
            row_best(A + 9 * r, col_used, v, c);
            if (v > best) { best = v; pr = r; pc = c; }
        }
        if (!(best >= kPivotMin)) return false;
        row_used |= 1U << pr; col_used |= 1U << pc; prow |= (uint32_t)pr << (4 * i); pcol |= (uint32_t)pc << (4 * i);
        for (int r = 0; r < kSample; r++) if (!((row_used >> r) & 1U)) row_eliminate(A + 9 * r, A + 9 * pr, pc, col_used);
    }
    double x[9];
    back_substitute(A, prow, pcol, col_used, x);
    denormalise(x, cax, cay, sa, cbx, cby, sb, F);
    return true;
}

// The whole stage on one set of n rows (n <= kMaxCandidates): pairs[i] is row i's virtual pixels, status[i] its status byte, rewritten in place.
// scratch: room for n Cand and n ints.  threshold: F_threshold in virtual pixels.
inline Result reject(const Cand* pairs, uint8_t* status, int n, double threshold, uint32_t seed, Cand* cand, int* row_of) {
    Result res{0, 0, -1, 0};
    int m = 0;
    for (int i = 0; i < n; i++) {
        if (!status[i]) continue;
        if (!finite_cand(pairs[i])) { status[i] = 0; res.rejected++; continue; }
        cand[m] = pairs[i]; row_of[m] = i; m++;
    }
    res.m = m;
    if (m < kSample) return res;
    const double tt = threshold * threshold;
    double best_F[9];
    for (int h = 0; h < kHypotheses; h++) {
        double F[9];
        if (!model(cand, m, seed, h, F)) continue;
        int count = 0;
        for (int j = 0; j < m; j++) count += inlier(F, cand[j], tt) ? 1 : 0;
        if (count >= kSample && count > res.inliers) { res.inliers = count; res.winner = h; for (int c = 0; c < 9; c++) best_F[c] = F[c]; }
    }
    if (res.winner < 0) return res;
    for (int j = 0; j < m; j++) if (!inlier(best_F, cand[j], tt)) { status[row_of[j]] = 0; res.rejected++; }
    return res;
}

// a setter's and the building blocks' check of one configuration; the reason into msg, naming the field
inline bool check_cfg(double f_threshold, double focal_length, char* msg, size_t len) {
    if (!(f_threshold - f_threshold == 0.0) || !(f_threshold > 0.0)) { snprintf(msg, len, "f_threshold %g (must be finite and > 0)", f_threshold); return false; }
    if (!(focal_length - focal_length == 0.0) || focal_length < 0.0) { snprintf(msg, len, "focal_length %g (must be finite and >= 0; 0 means %g)", focal_length, kFocal); return false; }
    return true;
}

}  // namespace gfrf
