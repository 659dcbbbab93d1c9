// gf_seq_size.hpp — the frame size a sequence of a tracker handle may have of its own (gf_tracker_set_seq_size, include/groundfusion_hip.h): `row`, `col` of
// FeatureTracker::trackImage (feature_tracker.cpp:108-109) per sequence.  Plain C++, no HIP types: the limits the setter checks, the pyramid geometry of a size,
// the table of the sizes in force on a handle and the plan of a call -- which size each list position has, the compact per-size tables of the launches whose
// form follows the size, and where each frame of a tight block lies -- in one place that the setter, the track calls and a stand-alone host program
// (tests/native/seq_size_host.cpp) share.
//
// The handle's cfg is the capacity: a sequence's two pyramid slots, its rows of every table and its share of the frame buffers stay where they are and as large
// as they are, and a smaller geometry lives inside them.  A size is one row of the handle's table of at most GF_MAX_SEQ_SIZES rows; row 0 is the handle's own
// size and never leaves.  The kernels that serve all sizes in one launch read a byte per list position that names the row (Plan::row); the launches whose form
// follows the size (the pyramid, the conversion, CLAHE, the track image) run once per distinct size of the call over that size's members, addressed through compact tables (Plan::member).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/groundfusion_hip.h"

namespace gfsize {

constexpr int kPad = 32, kWin = 21, kMaxLevels = 4;   // gf_lk_kernels.hpp (gf_tracker.hip holds the two sets of constants and the two structs together)
constexpr int kMinSide = 32;                          // gf_tracker_create's limits: width, height >= 32, width % 4 == 0

struct Level { int w, h, stride, img_off; };
struct Geom { Level lv[kMaxLevels]; int nlevels; size_t img_bytes; };   // PyrGeom (gf_lk_kernels.hpp), field for field

// build_geom (gf_tracker.hip) for a frame of w x h: buildOpticalFlowPyramid's levels inside one pyramid slot.  Every term grows with w and h.
inline void build_geom(int w, int h, Geom& G) {
    G = Geom{};
    int lw = w, lh = h, level = 0;
    size_t off = 0;
    for (; level < kMaxLevels; level++) {
        Level& g = G.lv[level];
        g.w = lw; g.h = lh; g.stride = lw + 2 * kPad;
        g.img_off = (int)(off + (size_t)kPad * g.stride + kPad);
        off += (size_t)(lh + 2 * kPad) * g.stride;
        off = (off + 255) & ~(size_t)255;
        lw = (lw + 1) / 2; lh = (lh + 1) / 2;
        if (lw <= kWin || lh <= kWin) { level++; break; }
    }
    G.nlevels = level;
    G.img_bytes = off;
}

// True if a sequence of a W x H handle can have w x h; otherwise a message that names the field.
inline bool limits_ok(int W, int H, int w, int h, char* msg, size_t n) {
    if (w < kMinSide || w > W) { snprintf(msg, n, "width %d is outside %d .. %d (gf_tracker_cfg.width is the capacity)", w, kMinSide, W); return false; }
    if (h < kMinSide || h > H) { snprintf(msg, n, "height %d is outside %d .. %d (gf_tracker_cfg.height is the capacity)", h, kMinSide, H); return false; }
    if (w % 4) { snprintf(msg, n, "width %d is no multiple of 4", w); return false; }
    return true;
}
// the pyramid of w x h lies inside a slot made for W x H
inline bool fits_slot(int w, int h, int W, int H) {
    Geom own, slot;
    build_geom(w, h, own); build_geom(W, H, slot);
    return own.img_bytes <= slot.img_bytes;
}

// The sizes in force on a handle.  Row 0 is the handle's own; the other rows are taken by the first sequence that is given a size no row holds and freed by the
// last that leaves it.  row_of[seq]: the row of each sequence.
struct Table {
    int w[GF_MAX_SEQ_SIZES] = {}, h[GF_MAX_SEQ_SIZES] = {}, users[GF_MAX_SEQ_SIZES] = {};
    std::vector<uint8_t> row_of;
    void init(int W, int H, int batch) {
        for (int r = 0; r < GF_MAX_SEQ_SIZES; r++) w[r] = h[r] = users[r] = 0;
        w[0] = W; h[0] = H; users[0] = batch;
        row_of.assign((size_t)batch, 0);
    }
    int in_force() const { int n = 1; for (int r = 1; r < GF_MAX_SEQ_SIZES; r++) n += users[r] > 0; return n; }
    // The row sequence `seq` would move to for ww x hh ((0, 0): the handle's): the row that holds the size, else a free one, else -1 -- a ninth distinct size.
    // The sequence's own row counts as free if it is its only user.  Changes nothing.
    int find(int seq, int ww, int hh) const {
        if (ww == 0 && hh == 0) return 0;
        for (int r = 0; r < GF_MAX_SEQ_SIZES; r++) if ((r == 0 || users[r] > 0) && w[r] == ww && h[r] == hh) return r;
        const int cur = row_of[(size_t)seq];
        if (cur != 0 && users[cur] == 1) return cur;
        for (int r = 1; r < GF_MAX_SEQ_SIZES; r++) if (users[r] == 0) return r;
        return -1;
    }
    void move(int seq, int r, int ww, int hh) {   // r from find()
        users[row_of[(size_t)seq]]--;
        if (r != 0) { w[r] = ww; h[r] = hh; }
        users[r]++;
        row_of[(size_t)seq] = (uint8_t)r;
    }
};

// The plan of one call.  Indexed by the list position i unless it says otherwise; the vectors keep their capacity from call to call.
struct Plan {
    int count = 0;
    bool sized = false;               // a listed sequence has a size that is not the handle's: the call takes the sized forms; else the code path of a handle without sizes
    std::vector<uint8_t> row;         // the table row of position i: what the sized kernels read by list position
    std::vector<int> w, h;
    std::vector<size_t> gray_off, depth_off, mask_off;   // bytes from the start of a tight block of frames / u16 depth frames / u8 masks: the sum of those listed before i
    size_t gray_bytes = 0, depth_bytes = 0, mask_bytes = 0;
    int max_w = 0, max_h = 0;         // the largest listed width and height: the grid of the one-launch kernels
    // The distinct sizes of the call in the order of their first appearance, and their members in list order: group g is row group_row[g] and the list positions
    // member[group_first[g] .. group_first[g] + group_n[g]).  Entry k of a compact table belongs to list position member[k].
    int n_groups = 0;
    int group_row[GF_MAX_SEQ_SIZES] = {}, group_first[GF_MAX_SEQ_SIZES] = {}, group_n[GF_MAX_SEQ_SIZES] = {};
    std::vector<int> member;
};

// bpp: bytes per pixel of the gray frame at each list position (its pixel format), or null: 1 everywhere
inline void plan_list(Plan& p, const Table& t, int count, const int* seq, const int* bpp = nullptr) {
    p.count = count; p.sized = false; p.n_groups = 0; p.max_w = p.max_h = 0;
    p.gray_bytes = p.depth_bytes = p.mask_bytes = 0;
    p.row.resize((size_t)count); p.w.resize((size_t)count); p.h.resize((size_t)count);
    p.gray_off.resize((size_t)count); p.depth_off.resize((size_t)count); p.mask_off.resize((size_t)count); p.member.resize((size_t)count);
    int group_of[GF_MAX_SEQ_SIZES];
    for (int r = 0; r < GF_MAX_SEQ_SIZES; r++) { group_of[r] = -1; p.group_n[r] = 0; }
    for (int i = 0; i < count; i++) {
        const int r = t.row_of[(size_t)seq[i]];
        p.row[i] = (uint8_t)r; p.w[i] = t.w[r]; p.h[i] = t.h[r];
        if (r != 0) p.sized = true;
        if (p.w[i] > p.max_w) p.max_w = p.w[i];
        if (p.h[i] > p.max_h) p.max_h = p.h[i];
        const size_t px = (size_t)p.w[i] * (size_t)p.h[i];
        p.gray_off[i] = p.gray_bytes; p.gray_bytes += px * (size_t)(bpp ? bpp[i] : 1);
        p.depth_off[i] = p.depth_bytes; p.depth_bytes += px * 2;
        p.mask_off[i] = p.mask_bytes; p.mask_bytes += px;
        if (group_of[r] < 0) { group_of[r] = p.n_groups; p.group_row[p.n_groups++] = r; }
        p.group_n[group_of[r]]++;
    }
    int at = 0;
    for (int g = 0; g < p.n_groups; g++) { p.group_first[g] = at; at += p.group_n[g]; p.group_n[g] = 0; }
    for (int i = 0; i < count; i++) {
        const int g = group_of[p.row[i]];
        p.member[(size_t)(p.group_first[g] + p.group_n[g]++)] = i;
    }
}

}  // namespace gfsize
