// gf_track_draw.hpp — the track image (FeatureTracker::drawTrack / getTrackImage, feature_tracker.cpp:849-905, :1047): the grey frame with one dot per feature,
// coloured from blue to red by track length, and a green arrow back to where the feature was one frame earlier.  One copy of what host and device share
// ("Track image"): the record of a primitive, the builder of a frame's list, the coverage predicates in exact integers, the per-pixel
// resolve and the tile-binning test of the kernel (gf_track_draw_kernels.hpp).  Plain C++: tests/native/track_draw_host.cpp renders whole frames with it on the CPU.
//
// The geometry, colours, order and rounding are the reference's; OpenCV's thick-circle and thick-line outlines are replaced by distance tests:
//   dot     (cv::circle, radius 2, thickness 6)      pixels with dx^2 + dy^2 <= 25 around the rounded centre
//   stroke  (one line of cv::arrowedLine, thickness 3) pixels whose squared distance to the segment is <= 9/4
//   frame   (drawTrackbox's cv::rectangle of a box, thickness 5, feature_tracker.cpp:960-975)  the pixels within 2 of the rectangle's outline, three inequalities
// (0, 128, 255) where any box's frame covers, else green where any stroke covers, else the colour of the covering dot with the largest list index, else (g, g, g).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/groundfusion_hip.h"   // gf_box

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define GF_DRAW_HD __host__ __device__ __forceinline__
#else
#define GF_DRAW_HD inline
#endif

namespace gfdraw {

constexpr int kDotR2 = 25;             // dx^2 + dy^2 <= 25: 81 pixels
constexpr int kDotReach = 5;           // ... none further than 5 from the centre along an axis
constexpr int kStrokeReach = 1;        // 4 d^2 <= 9 on integer offsets: none further than 1 from the segment's bounding box
constexpr int kMaxCoord = 1 << 20;     // |x|, |y| of a point handed to build_list
constexpr int kTrackFull = 20;         // len = min(1, track_cnt / 20)

// Scalar(255 * (1 - len), 0, 255 * len) for track_cnt = 0 .. 20, the reference's expression in double rounded by lrint (saturate_cast<uchar>(double)), as
// literals: 255 * (1 - 14 / 20.) is 76.50000000000001 and gives 77, the same expression at 18 is 25.499999999999993 and gives 25.
GF_DRAW_HD uint8_t color0(int k) {
    constexpr uint8_t t[kTrackFull + 1] = {255, 242, 230, 217, 204, 191, 178, 166, 153, 140, 128, 115, 102, 89, 77, 64, 51, 38, 25, 13, 0};
    return t[k];
}
GF_DRAW_HD uint8_t color2(int k) {
    constexpr uint8_t t[kTrackFull + 1] = {0, 13, 26, 38, 51, 64, 76, 89, 102, 115, 128, 140, 153, 166, 178, 191, 204, 217, 230, 242, 255};
    return t[k];
}

// One primitive.  A dot: centre (ux, uy), colour bytes (c0, 0, c2); vx, vy unused (0).  A stroke (stroke == 1): the segment (ux, uy) - (vx, vy), always (0, 255, 0).
// A frame (stroke == kFrame): the rectangle of pixels X0 = ux .. X1 = vx, Y0 = uy .. Y1 = vy whose outline is drawn 5 wide, always (0, 128, 255).
struct Prim { int32_t ux, uy, vx, vy; uint8_t stroke, c0, c2, pad; };
constexpr uint8_t kFrame = 2;
constexpr int kFrameReach = 2;         // a frame reaches 2 pixels outside and inside its rectangle's outline
static_assert(sizeof(Prim) == 20, "Prim is copied to the device as it lies");

GF_DRAW_HD Prim make_dot(int x, int y, int track_cnt) {
    const int k = track_cnt < kTrackFull ? track_cnt : kTrackFull;
    return Prim{x, y, 0, 0, 0, color0(k), color2(k), 0};
}
GF_DRAW_HD Prim make_stroke(int ux, int uy, int vx, int vy) { return Prim{ux, uy, vx, vy, 1, 0, 255, 0}; }
// The frame of a box: cv::rectangle(img, Rect(xmin, ymin, xmax - xmin, ymax - ymin), Scalar(0, 128, 255), 5).  False, and nothing is drawn, unless xmax > xmin &&
// ymax > ymin (an empty cv::Rect).  X1 = xmax - 1 and Y1 = ymax - 1 in 64 bits, then every coordinate clamped to +-kMaxCoord: a frame's pixels inside an image
// (coordinates 0 .. < 2^20 - 2) are the same with the clamped corners as with the box's own.
GF_DRAW_HD int32_t clamp_coord(int64_t v) { return (int32_t)(v < -kMaxCoord ? -kMaxCoord : v > kMaxCoord ? kMaxCoord : v); }
GF_DRAW_HD bool make_frame(const gf_box& b, Prim& out) {
    if (!(b.xmax > b.xmin && b.ymax > b.ymin)) return false;
    out = Prim{clamp_coord(b.xmin), clamp_coord(b.ymin), clamp_coord((int64_t)b.xmax - 1), clamp_coord((int64_t)b.ymax - 1), kFrame, 0, 255, 0};
    return true;
}

// ---- coverage, in exact integers.  A dot's centre and a stroke's ends lie within 2^21 of the origin (build_list: points within 2^20, tips within 0.2 * the
// arrow's length of one), pixels inside an image: every difference is below 2^23, every dot product and L below 2^47.
GF_DRAW_HD bool dot_covers(const Prim& p, int x, int y) {
    const int64_t dx = (int64_t)x - p.ux, dy = (int64_t)y - p.uy;
    return dx * dx + dy * dy <= kDotR2;
}
GF_DRAW_HD bool stroke_covers(const Prim& s, int x, int y) {
    const int64_t dx = (int64_t)s.vx - s.ux, dy = (int64_t)s.vy - s.uy, px = (int64_t)x - s.ux, py = (int64_t)y - s.uy;
    const int64_t L = dx * dx + dy * dy, t = px * dx + py * dy;
    if (t <= 0) return 4 * (px * px + py * py) <= 9;          // also the stroke of no length: the 3 x 3 block
    if (t >= L) { const int64_t qx = (int64_t)x - s.vx, qy = (int64_t)y - s.vy; return 4 * (qx * qx + qy * qy) <= 9; }
    int64_t cr = px * dy - py * dx;
    if (cr < 0) cr = -cr;
    // 4 cr^2 <= 9 L.  cr^2 itself can pass 2^63; but 9 L < 2^51, so a |cr| of 2^25 or more (4 cr^2 >= 2^52) is outside whatever L is, and below it 4 cr^2 < 2^52.
    if (cr >= ((int64_t)1 << 25)) return false;
    return 4 * cr * cr <= 9 * L;
}
// the frame of X0 = ux .. X1 = vx, Y0 = uy .. Y1 = vy (|coordinates| <= 2^20: the sums below stay far inside 32 bits)
GF_DRAW_HD bool frame_covers(const Prim& f, int x, int y) {
    if (x < f.ux - kFrameReach || x > f.vx + kFrameReach || y < f.uy - kFrameReach || y > f.vy + kFrameReach) return false;
    return !(x > f.ux + kFrameReach && x < f.vx - kFrameReach && y > f.uy + kFrameReach && y < f.vy - kFrameReach);
}
GF_DRAW_HD bool covers(const Prim& p, int x, int y) { return p.stroke == kFrame ? frame_covers(p, x, y) : p.stroke ? stroke_covers(p, x, y) : dot_covers(p, x, y); }

// ---- binning: whether a primitive can cover a pixel of the rectangle x0 .. x1, y0 .. y1 (inclusive), by its bounding box.  Never false for a primitive that
// covers one (tests/native/track_draw_host.cpp holds it to brute force); what it lets through in vain costs the kernel time only.
GF_DRAW_HD bool touches(const Prim& p, int x0, int y0, int x1, int y1) {
    int lx, hx, ly, hy;
    if (p.stroke == kFrame) {   // also not a tile that lies wholly in the frame's open inside
        if (x0 > p.ux + kFrameReach && x1 < p.vx - kFrameReach && y0 > p.uy + kFrameReach && y1 < p.vy - kFrameReach) return false;
        lx = p.ux - kFrameReach; hx = p.vx + kFrameReach; ly = p.uy - kFrameReach; hy = p.vy + kFrameReach;
    } else if (p.stroke) {
        lx = (p.ux < p.vx ? p.ux : p.vx) - kStrokeReach; hx = (p.ux < p.vx ? p.vx : p.ux) + kStrokeReach;
        ly = (p.uy < p.vy ? p.uy : p.vy) - kStrokeReach; hy = (p.uy < p.vy ? p.vy : p.uy) + kStrokeReach;
    } else { lx = p.ux - kDotReach; hx = p.ux + kDotReach; ly = p.uy - kDotReach; hy = p.uy + kDotReach; }
    return lx <= x1 && hx >= x0 && ly <= y1 && hy >= y0;
}

// ---- the per-pixel resolve.  A pixel walks the primitives that may cover it, in any order and in any number of pieces, and keeps: whether a stroke covered it,
// whether a frame did (frames cover strokes and dots, and all frames have one colour, so a later one covering an earlier one changes no byte), and the covering
// dot of the largest list index.  The result is a function of the list alone.
struct Acc { int32_t dot; uint8_t green, c0, c2, frame; };   // dot: list index of the dot kept so far, -1: none
GF_DRAW_HD Acc acc_empty() { return Acc{-1, 0, 0, 0, 0}; }
GF_DRAW_HD void accumulate(Acc& a, const Prim& p, int index, int x, int y) {
    if (p.stroke == kFrame) { if (!a.frame && frame_covers(p, x, y)) a.frame = 1; }
    else if (p.stroke) { if (!a.green && stroke_covers(p, x, y)) a.green = 1; }
    else if (index > a.dot && dot_covers(p, x, y)) { a.dot = index; a.c0 = p.c0; a.c2 = p.c2; }
}
// the pixel's three bytes in memory order, as c0 | c1 << 8 | c2 << 16
GF_DRAW_HD uint32_t finish(const Acc& a, uint8_t g) {
    if (a.frame) return (128u << 8) | (255u << 16);   // Scalar(0, 128, 255)
    if (a.green) return 255u << 8;
    if (a.dot >= 0) return (uint32_t)a.c0 | ((uint32_t)a.c2 << 16);
    return (uint32_t)g * 0x010101u;
}
GF_DRAW_HD uint32_t resolve(const Prim* list, int n, int x, int y, uint8_t g) {
    Acc a = acc_empty();
    for (int i = 0; i < n; i++) accumulate(a, list[i], i, x, y);
    return finish(a, g);
}

// ---- the list of one frame (host only: the arrow tips go through the C library's atan2 / cos / sin in double, so no device transcendental decides a pixel).
// cur_xy / prev_xy: n points as x, y pairs; has_prev[i]: feature i was tracked into this frame from prev_xy[i] (not read otherwise; prev_xy and has_prev may be
// null: no arrows).  out: room for list_capacity(n) primitives -- all dots in list order, then the arrows' strokes.  Returns the number written, or -1 with the
// reason in msg: a track_cnt < 0, a point that is not finite or beyond 2^20 in magnitude.
inline size_t list_capacity(size_t n) { return 4 * n; }
// the frames of the boxes in force, appended behind a frame's dots and strokes (drawTrackbox draws them last, :960-975); returns how many were written (<= n)
inline int append_frames(const gf_box* boxes, int n, Prim* out) {
    int m = 0;
    for (int i = 0; i < n; i++) if (make_frame(boxes[i], out[m])) m++;
    return m;
}
inline bool point_ok(float x, float y) { return isfinite(x) && isfinite(y) && fabsf(x) <= (float)kMaxCoord && fabsf(y) <= (float)kMaxCoord; }
inline int build_list(int n, const float* cur_xy, const int* track_cnt, const float* prev_xy, const uint8_t* has_prev, Prim* out, char* msg, size_t msg_len) {
    for (int i = 0; i < n; i++) {
        if (track_cnt[i] < 0) { snprintf(msg, msg_len, "feature %d has track_cnt %d", i, track_cnt[i]); return -1; }
        if (!point_ok(cur_xy[2 * i], cur_xy[2 * i + 1])) { snprintf(msg, msg_len, "feature %d lies at (%g, %g): not finite or beyond 2^20", i, (double)cur_xy[2 * i], (double)cur_xy[2 * i + 1]); return -1; }
        if (has_prev && prev_xy && has_prev[i] && !point_ok(prev_xy[2 * i], prev_xy[2 * i + 1])) {
            snprintf(msg, msg_len, "feature %d came from (%g, %g): not finite or beyond 2^20", i, (double)prev_xy[2 * i], (double)prev_xy[2 * i + 1]); return -1;
        }
    }
    int m = 0;
    for (int i = 0; i < n; i++) out[m++] = make_dot((int)lrintf(cur_xy[2 * i]), (int)lrintf(cur_xy[2 * i + 1]), track_cnt[i]);   // Point2f -> Point: round half to even
    if (!has_prev || !prev_xy) return m;
    for (int i = 0; i < n; i++) {
        if (!has_prev[i]) continue;
        // cv::arrowedLine(img, pt1 = cur, pt2 = prev, .., tipLength = 0.2): the head sits at prev
        const int ax = (int)lrintf(cur_xy[2 * i]), ay = (int)lrintf(cur_xy[2 * i + 1]), bx = (int)lrintf(prev_xy[2 * i]), by = (int)lrintf(prev_xy[2 * i + 1]);
        const double ddx = (double)ax - bx, ddy = (double)ay - by;
        const double tip = 0.2 * sqrt(ddx * ddx + ddy * ddy), ang = atan2(ddy, ddx);
        const double quarter = 3.14159265358979323846 / 4;
        out[m++] = make_stroke(ax, ay, bx, by);
        out[m++] = make_stroke((int)lrint(bx + tip * cos(ang + quarter)), (int)lrint(by + tip * sin(ang + quarter)), bx, by);
        out[m++] = make_stroke((int)lrint(bx + tip * cos(ang - quarter)), (int)lrint(by + tip * sin(ang - quarter)), bx, by);
    }
    return m;
}

// One frame of a launch of the kernel, every address resolved by the host: the MONO8 background, the destination (written), the frame's list.
struct DrawJob { const uint8_t* gray; size_t gray_pitch; uint8_t* dst; size_t dst_pitch; const Prim* prims; int n; int pad; };

// a whole frame on the CPU by the same per-pixel function (the yardstick of the host tests; the library renders on the device only)
inline void render_host(const uint8_t* gray, size_t gray_pitch, int w, int h, const Prim* list, int n, uint8_t* dst, size_t dst_pitch) {
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const uint32_t v = resolve(list, n, x, y, gray[(size_t)y * gray_pitch + x]);
            uint8_t* o = dst + (size_t)y * dst_pitch + 3 * (size_t)x;
            o[0] = (uint8_t)v; o[1] = (uint8_t)(v >> 8); o[2] = (uint8_t)(v >> 16);
        }
}

}  // namespace gfdraw
