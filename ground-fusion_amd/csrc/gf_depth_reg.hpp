// gf_depth_reg.hpp — raw depth registered to the colour camera (gf_depth_reg; gf_tracker_set_seq_depth_reg, gf_depth_register_batch*): what the camera driver's
// `align` filter does on the host for /camera/aligned_depth_to_color/image_raw, as a definition of this repository ("Depth registration").
// Plain C++ in double precision that host and device both compile, one source for the scatter kernel (gf_depth_reg_kernels.hpp), the tracker's setter and the
// stand-alone host program of the tests (tests/native/depth_reg_host.cpp).  It sets no floating-point contraction of its own; the library compiles it without
// contraction on both sides, and nothing here but +, -, *, /, floor, ceil and comparisons touches a double, so host and device give the same bits.
//
// One depth pixel (x, y) with count d != 0, z = (double)d * scale:
//   map(px, py):  X = (px - cx_d) / fx_d * z,  Y = (py - cy_d) / fy_d * z,  P = R (X, Y, z) + T with each row summed as ((R0 X + R1 Y) + R2 z) + T;
//                 !(P.z > 0): nothing.  (u, v) = gfcam::distort_to_plane(colour pinhole, P.x / P.z, P.y / P.z) -- the projection setPrediction uses -- or, for a
//                 PINHOLE_FULL colour camera, gfcam::full_distort_to_plane, the tail of that model's spaceToPlane.  Nothing else depends on the model.
//   a = map(x - 0.5, y - 0.5), b = map(x + 0.5, y + 0.5), c = map(x, y); one of them behind the camera or a coordinate that is not finite: nothing.
//   val = floor(c.Pz / 0.001 + 0.5), millimetres along the colour camera's axis; outside [1, 65535]: nothing.
//   footprint: the colour pixels whose centre lies in the half-open box of the corners, x0 = ceil(min(a.u, b.u)), x1 = ceil(max(a.u, b.u)) - 1, y alike;
//   wider or higher than kMaxFoot pixels: nothing; else clipped to the colour frame (may come out empty).
// A colour pixel takes the smallest val among the footprints that hold it, 0 if none does.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/groundfusion_hip.h"   // gf_depth_reg, gf_camera_model
#include "gf_camera_models.hpp"               // gfcam::distort_to_plane, gfcam::full_distort_to_plane

#if defined(__HIPCC__) || defined(__HIP__)
#define GF_DREG_HD __host__ __device__ inline
#else
#define GF_DREG_HD inline
#endif

namespace gfdreg {

constexpr int kMaxFoot = 8;                   // a footprint wider or higher than this contributes nothing: the bound of every loop
constexpr uint32_t kUntouched = 0xFFFFFFFFu;  // what the z-buffer holds where no footprint arrived
constexpr int kMinSize = 8, kMaxSize = 4096;

// One registration as map() reads it.  The first 25 doubles: the depth pinhole, the scale, the pose, the colour pinhole with its distortion -- all a PINHOLE
// colour camera has.  Behind them what a PINHOLE_FULL one adds: k3 .. k6 and the model, which map<false> never reads.
struct Params { double fxd, fyd, cxd, cyd, scale, R[9], T[3], fx, fy, cx, cy, k1, k2, p1, p2; double k3, k4, k5, k6; int32_t model, reserved; };
constexpr int kPinholeDoubles = 25;
static_assert(offsetof(Params, k3) == kPinholeDoubles * sizeof(double) && sizeof(Params) == 30 * sizeof(double), "Params is 25 doubles and the PINHOLE_FULL tail, read as such by the kernel");

struct Mapped { double u, v, Pz; };
// rule 2.  False: the point is not in front of the colour camera.  FULL: the entry may be a PINHOLE_FULL one (a branch on its model, the same for every pixel of
// the entry); without, p is a PINHOLE entry and its tail is not read.
template <bool FULL = true> GF_DREG_HD bool map(const Params& p, double px, double py, double z, Mapped& m) {
    const double X = (px - p.cxd) / p.fxd * z;
    const double Y = (py - p.cyd) / p.fyd * z;
    const double Px = ((p.R[0] * X + p.R[1] * Y) + p.R[2] * z) + p.T[0];
    const double Py = ((p.R[3] * X + p.R[4] * Y) + p.R[5] * z) + p.T[1];
    const double Pz = ((p.R[6] * X + p.R[7] * Y) + p.R[8] * z) + p.T[2];
    if (!(Pz > 0.0)) return false;
    if (FULL && p.model == GF_CAMERA_PINHOLE_FULL) gfcam::full_distort_to_plane(p.fx, p.fy, p.cx, p.cy, p.k1, p.k2, p.p1, p.p2, p.k3, p.k4, p.k5, p.k6, Px / Pz, Py / Pz, m.u, m.v);
    else gfcam::distort_to_plane(p.fx, p.fy, p.cx, p.cy, p.k1, p.k2, p.p1, p.p2, Px / Pz, Py / Pz, m.u, m.v);
    m.Pz = Pz;
    return true;
}
GF_DREG_HD bool finite(double v) { return fabs(v) <= 1.7976931348623157e308; }   // false for NaN too

// What became of a depth pixel, in the order the rules are applied.
enum Outcome { kZero = 0, kBehind, kNotFinite, kOutOfRange, kOverBound, kEmpty, kWrites };
struct Foot { int x0, x1, y0, y1; uint32_t val; };   // inclusive, inside the colour frame
// rules 1-5 for the depth pixel (x, y) with count d into a colour frame of wc x hc
template <bool FULL = true> GF_DREG_HD Outcome footprint(const Params& p, int wc, int hc, int x, int y, uint16_t d, Foot& f) {
    if (d == 0) return kZero;
    const double z = (double)d * p.scale;
    Mapped a, b, c;
    if (!map<FULL>(p, (double)x - 0.5, (double)y - 0.5, z, a) || !map<FULL>(p, (double)x + 0.5, (double)y + 0.5, z, b) || !map<FULL>(p, (double)x, (double)y, z, c)) return kBehind;
    if (!finite(a.u) || !finite(a.v) || !finite(b.u) || !finite(b.v) || !finite(c.u) || !finite(c.v)) return kNotFinite;
    const double val = floor(c.Pz / 0.001 + 0.5);
    if (!(val >= 1.0 && val <= 65535.0)) return kOutOfRange;
    double x0 = ceil(a.u < b.u ? a.u : b.u), x1 = ceil(a.u < b.u ? b.u : a.u) - 1.0;
    double y0 = ceil(a.v < b.v ? a.v : b.v), y1 = ceil(a.v < b.v ? b.v : a.v) - 1.0;
    if (x1 - x0 + 1.0 > (double)kMaxFoot || y1 - y0 + 1.0 > (double)kMaxFoot) return kOverBound;
    if (x0 < 0.0) x0 = 0.0;
    if (y0 < 0.0) y0 = 0.0;
    if (x1 > (double)(wc - 1)) x1 = (double)(wc - 1);
    if (y1 > (double)(hc - 1)) y1 = (double)(hc - 1);
    if (x0 > x1 || y0 > y1) return kEmpty;
    f.x0 = (int)x0; f.x1 = (int)x1; f.y0 = (int)y0; f.y1 = (int)y1; f.val = (uint32_t)val;   // all inside the frame after the clip: the conversions are exact
    return kWrites;
}

// What a thread of the scatter kernel does with its depth pixel: rule 6 into a z-buffer of rows `zstride` words apart.  min_into(word, val): the device's atomic
// minimum, the host's plain one.  At most kMaxFoot x kMaxFoot calls.
template <bool FULL = true, class MIN> GF_DREG_HD Outcome scatter_pixel(const Params& p, int wc, int hc, int x, int y, uint16_t d, uint32_t* z, size_t zstride, MIN min_into) {
    Foot f;
    const Outcome o = footprint<FULL>(p, wc, hc, x, y, d, f);
    if (o != kWrites) return o;
    for (int v = f.y0; v <= f.y1; v++)
        for (int u = f.x0; u <= f.x1; u++) min_into(z + (size_t)v * zstride + u, f.val);
    return o;
}
// What the finish kernel does with a word: the u16 of the output, 0 where nothing arrived.  (Every val is in [1, 65535].)
GF_DREG_HD uint16_t narrow(uint32_t word) { return word == kUntouched ? (uint16_t)0 : (uint16_t)word; }
// rows of the z-buffer start on 32 bytes, so that the finish kernel reads and re-primes eight words per lane whatever the width
GF_DREG_HD size_t zstride_of(int wc) { return ((size_t)wc + 7) & ~(size_t)7; }

// One frame on the host, by walking the depth pixels: the CPU form of the two kernels.  src / dst: rows src_pitch / dst_pitch BYTES apart; z: hc rows of
// zstride_of(wc) words holding kUntouched, left so.  Of dst only wc counts of each of hc rows are written.  census (may be null): [kWrites + 1] counts by Outcome.
inline void register_frame(const Params& p, const void* src, size_t src_pitch, int wd, int hd, void* dst, size_t dst_pitch, int wc, int hc, uint32_t* z, long long* census = nullptr) {
    const size_t zs = zstride_of(wc);
    for (int y = 0; y < hd; y++) {
        const uint16_t* row = reinterpret_cast<const uint16_t*>(static_cast<const uint8_t*>(src) + (size_t)y * src_pitch);
        for (int x = 0; x < wd; x++) {
            const Outcome o = scatter_pixel(p, wc, hc, x, y, row[x], z, zs, [](uint32_t* w, uint32_t v) { if (v < *w) *w = v; });
            if (census) census[o]++;
        }
    }
    for (int v = 0; v < hc; v++) {
        uint16_t* row = reinterpret_cast<uint16_t*>(static_cast<uint8_t*>(dst) + (size_t)v * dst_pitch);
        for (int u = 0; u < wc; u++) { row[u] = narrow(z[(size_t)v * zs + u]); z[(size_t)v * zs + u] = kUntouched; }
    }
}

// ---- host side: what a setter checks
// False with a message that names the field: a size outside kMinSize .. kMaxSize, a value that is not finite, fx, fy or scale <= 0, an R with
// |R R^T - I| > 1e-6 in an entry or det R <= 0.
inline bool check(const gf_depth_reg& r, char* msg, size_t n) {
    if (r.width < kMinSize || r.width > kMaxSize) { snprintf(msg, n, "gf_depth_reg.width %d is outside %d .. %d", r.width, kMinSize, kMaxSize); return false; }
    if (r.height < kMinSize || r.height > kMaxSize) { snprintf(msg, n, "gf_depth_reg.height %d is outside %d .. %d", r.height, kMinSize, kMaxSize); return false; }
    const double v[5] = {r.fx, r.fy, r.cx, r.cy, r.scale};
    static const char* const name[5] = {"fx", "fy", "cx", "cy", "scale"};
    for (int i = 0; i < 5; i++) if (!finite(v[i])) { snprintf(msg, n, "gf_depth_reg.%s is not finite", name[i]); return false; }
    for (int i = 0; i < 9; i++) if (!finite(r.R[i])) { snprintf(msg, n, "gf_depth_reg.R[%d] is not finite", i); return false; }
    for (int i = 0; i < 3; i++) if (!finite(r.T[i])) { snprintf(msg, n, "gf_depth_reg.T[%d] is not finite", i); return false; }
    if (!(r.fx > 0.0)) { snprintf(msg, n, "gf_depth_reg.fx must be > 0, got %g", r.fx); return false; }
    if (!(r.fy > 0.0)) { snprintf(msg, n, "gf_depth_reg.fy must be > 0, got %g", r.fy); return false; }
    if (!(r.scale > 0.0)) { snprintf(msg, n, "gf_depth_reg.scale must be > 0 (metres per count), got %g", r.scale); return false; }
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            const double e = r.R[3 * i] * r.R[3 * j] + r.R[3 * i + 1] * r.R[3 * j + 1] + r.R[3 * i + 2] * r.R[3 * j + 2] - (i == j ? 1.0 : 0.0);
            if (!(fabs(e) <= 1e-6)) { snprintf(msg, n, "gf_depth_reg.R is no rotation: (R R^T - I)[%d][%d] is %g, beyond 1e-6", i, j, e); return false; }
        }
    const double det = r.R[0] * (r.R[4] * r.R[8] - r.R[5] * r.R[7]) - r.R[1] * (r.R[3] * r.R[8] - r.R[5] * r.R[6]) + r.R[2] * (r.R[3] * r.R[7] - r.R[4] * r.R[6]);
    if (!(det > 0.0)) { snprintf(msg, n, "gf_depth_reg.R is a reflection: its determinant is %g", det); return false; }
    return true;
}

// a checked registration and a colour pinhole (proj = fx fy cx cy, dist = k1 k2 p1 p2), or with `full` (k3 k4 k5 k6) a colour PINHOLE_FULL
inline Params params_of(const gf_depth_reg& r, const double* proj, const double* dist, const double* full = nullptr) {
    Params p{};
    p.fxd = r.fx; p.fyd = r.fy; p.cxd = r.cx; p.cyd = r.cy; p.scale = r.scale;
    for (int i = 0; i < 9; i++) p.R[i] = r.R[i];
    for (int i = 0; i < 3; i++) p.T[i] = r.T[i];
    p.fx = proj[0]; p.fy = proj[1]; p.cx = proj[2]; p.cy = proj[3];
    p.k1 = dist[0]; p.k2 = dist[1]; p.p1 = dist[2]; p.p2 = dist[3];
    if (full) { p.k3 = full[0]; p.k4 = full[1]; p.k5 = full[2]; p.k6 = full[3]; p.model = GF_CAMERA_PINHOLE_FULL; }
    return p;
}

// ---- what the two kernels (gf_depth_reg_kernels.hpp) are launched with, for the translation units that launch them without holding them
// One list entry: a raw depth frame, where its registered frame goes, and where its rows of the z-buffer begin (words from the buffer's start, a multiple of 8).
struct alignas(8) Job {
    const uint8_t* src; size_t src_pitch;
    uint8_t* dst; size_t dst_pitch;
    size_t zoff;
    int32_t wd, hd, wc, hc;
    Params p;
};
static_assert(sizeof(Job) == 5 * 8 + 4 * 4 + sizeof(Params), "Job is read as dwords by the kernels");
inline size_t zwords_of(int wc, int hc) { return zstride_of(wc) * (size_t)hc; }

}  // namespace gfdreg
